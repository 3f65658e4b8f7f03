"""CPU: every batch of decode_inplace_cases.py reaches the route it is named for (the stream at a
16-B-aligned address, as test_gpu_decode_inplace.py places it), and the oracle decodes it."""
import pytest

import decode_cases as dc
import decode_inplace_cases as ic
from oracle import oracle as O


@pytest.fixture(scope="module")
def R():
    memo = {}

    def get(name):
        if name not in memo:
            b = ic.CASES[name]()
            memo[name] = (b, [r for r in ic.routes(b) if r[0] != "filler"])
        return memo[name]
    return get


def test_constants():
    assert ic.kDecImg + ic.kDecKeyImg + 2 * ic.kDecMapN <= (160 << 10) // 24  # 24 workgroups per CU
    assert ic.kDecKeyImg % 16 == 0 and ic.kDecOut <= 16 * ic.kDecMapN <= ic.kDecImg
    assert 4 * dc.C.kCopyScratch <= ic.kDecKeyImg  # the large-block path borrows the key image
    assert ic.kDecMB == 2 and ic.kDecMaxE == 128


@pytest.mark.parametrize("name", tuple(ic.CASES))
def test_oracle_decodes(R, name):
    b, _ = R(name)
    rc, kv = O.decode_blocks(b.blocks, b.blk_off)
    assert rc == 0 and kv.n == len(b.entries())


def test_align(R):
    _, rs = R("align")
    assert {(t, r) for t, r, _ in rs} == {(f"align:{ld}:{vb}", "inplace") for ld in range(16) for vb in range(16)}
    assert all((i["lead"], i["vb"]) == tuple(map(int, t.split(":")[1:])) and i["short"] == 1 and i["moved"] >= 7
               for t, _, i in rs)


def test_vlens(R):
    _, rs = R("vlens")
    assert [t for t, _, _ in rs] == [f"vlen:{vl}:{pos}" for vl in ic.VLENS for pos in (0, 2, 4)]
    assert all(r == "inplace" for _, r, _ in rs)
    assert all(i["short"] == (t.split(":")[1] == "15") for t, _, i in rs)


def test_first_keys(R):
    _, rs = R("first_keys")
    first1 = [(t, r, i) for t, r, i in rs if t.startswith("first1")]
    assert all(r == "inplace" and i["lead"] == 0 and i["first_s"] == 1 and i["d0"] == 15 - i["vb"] for _, r, i in first1)
    assert sorted(i["vb"] for t, _, i in first1 if t.startswith("first1:")) == list(range(16))
    assert {i["d0"] for _, _, i in first1} == set(range(16))  # 0: the value stays where it is
    got = {t: (r, i["kb"] + i["K"]) for t, r, i in rs if t.startswith("firstmax")}
    assert got == {f"firstmax:{kb}:{o}": ("glb:keys" if o > 0 else "inplace", ic.kDecKeyImg + o)
                   for kb in (0, 7, 15) for o in (-1, 0, 1)}


def test_key_image(R):
    _, rs = R("key_image")
    got = {t: (r, i["kb"] + i["K"]) for t, r, i in rs}
    assert got == {f"keyimg:{kb}:{o}": ("glb:keys" if o > 0 else "inplace", ic.kDecKeyImg + o)
                   for kb in (0, 3, 15) for o in (-17, -1, 0, 1)}


def test_out_bound(R):
    _, rs = R("out_bound")
    for t, r, i in rs:
        over = int(t.split(":")[3])
        assert i["krun"] + i["vb"] + i["V"] == ic.kDecOut + over and i["krun"] <= ic.kDecKeyImg
        assert r == ("glb:out" if over > 0 else "inplace"), t


def test_counts(R):
    _, rs = R("counts")
    assert [i["n"] for _, _, i in rs] == [n for n in ic.COUNTS for _ in range(2)]
    assert all(r == ("simple" if i["n"] > ic.kDecMaxE else "inplace") for _, r, i in rs)
    assert all(i["moved"] > 0 for _, _, i in rs)


def test_batches(R):
    _, rs = R("batches")
    assert all(r == "inplace" for _, r, _ in rs)
    assert sorted({i["whole"] for _, _, i in rs}) == [ic.BATCH // 2, ic.BATCH // 2 + 1, ic.BATCH, ic.BATCH + 1]
    assert (ic.BATCH // 2, ic.BATCH) == (64, 128)


def test_overlap(R):
    b, rs = R("overlap")
    assert len(rs) == 200 and all(r == "inplace" for _, r, _ in rs)
    assert sum(i["short"] > 0 for _, _, i in rs) > 50 and sum(i["zero"] > 0 for _, _, i in rs) > 20
    # neighbours share chunks: most blocks start and end inside a 16-B chunk of either arena
    assert sum(i["vb"] != 0 for _, _, i in rs) > 100 and sum(i["kb"] != 0 for _, _, i in rs) > 100
    assert len({len(x) % 16 for x in b.bufs}) == 16


def test_order(R):
    _, rs = R("order")
    got = {}
    for t, r, _ in rs:
        got.setdefault(t, set()).add(r)
    assert got == {"order:reversed": {"glb:order"}, "order:swap": {"glb:order"}, "order:twice": {"glb:order"},
                   "order:amplified": {"glb:order"}, "order:gaps": {"inplace"}}
