"""The plan-walk inputs of tests/walk_cases.py, checked on the CPU: every generator's stream is
oracle-encoded, the lane-level restatement of walk_segment must find the oracle's block table on it
(first entries and sizes, so every prefix it summed), and must report the lanes, windows, carries,
ring slots and reject-rule edges the generator was built for; the pair classifier must show every
route of the helper's LCP at every alignment of the key arena.  test_gpu_walk.py runs the same
inputs on the device."""
import numpy as np
import pytest

import path_cases as pc
import walk_cases as wc
from oracle import oracle as O


def encode(case, decodes=True):
    kv, seg, bs = case
    rc, blocks, off = O.encode_segments(kv, seg, bs)
    assert rc == 0
    if decodes:
        rc, back = O.decode_blocks(blocks, off)
        assert rc == 0 and pc.kv_equal(back, kv), "generator: the oracle does not read its own blocks back"
    return blocks, off


def walked(case, decodes=True, ring_base=None, pairs=None):
    """The restatement of the walk over the case, held against the oracle's block table."""
    blocks, off = encode(case, decodes)
    W = wc.Walk(*case, ring_base=ring_base, pairs=pairs)
    wc.check_table(W, blocks, off)
    return W


def test_constants_are_read_from_the_kernel_source(tmp_path):
    assert wc.kRing >= 2 * wc.kChunk and wc.kRing % wc.kPipeE == 0 and wc.kChunk % (64 * wc.kProdBatch) == 0
    assert wc.kAlcpLcp == (1 << 31) - 1 and wc.kHugeRec == wc.kGrowMax - 16 and wc.kNarrowBs == 1 << 30
    f = tmp_path / "k.hip"
    src = open(wc._SRC).read()
    f.write_text(src.replace("constexpr uint32_t kChunk", "constexpr uint32_t kChunkX"))
    with pytest.raises(RuntimeError):
        wc.walk_constants(str(f))
    f.write_text(src.replace("narrow = bs <", "narrow = bs <="))
    with pytest.raises(RuntimeError):
        wc.walk_constants(str(f))


def check_pair_probes(kv, seg, P):
    """Every probe one block's worth, every unsorted probe defeats the min shortcut, no sorted one does."""
    nun = 0
    for g in range(len(seg) - 1):
        s0, s1 = int(seg[g]), int(seg[g + 1])
        uns = (~P.sorted[s0:s1 - 1]).any()
        nun += int(uns)
        assert bool(wc.shortcut_differs(kv, P, s0, s1)) == bool(uns), f"probe {g} (unsorted: {uns})"
    return nun


def test_pair_probes():
    case = wc.pair_probes()
    kv, seg, bs = case
    blocks, off = encode(case)
    assert pc.one_block_per_segment(off, seg)
    want = {(r, s, q) for r in ("select", "dword") for s in (False, True) for q in range(4)}
    for glead in range(16):
        P = wc.classify_pairs(kv, seg, 256 + glead)
        assert want <= P.seen(), f"glead {glead}: missing {sorted(want - P.seen())}"
        assert not any(x[0] == "tail" for x in P.seen())
    nun = check_pair_probes(kv, seg, P)
    i = P.inside
    # first differences at every z, by every byte pair, in both orders; prefix pairs of every length
    for z in wc.FIRST_DIFF_Z:
        for lo, hi in wc.BYTE_PAIRS:
            assert (i & (P.z == z) & (P.b0 == lo) & (P.b1 == hi) & P.sorted).any(), (z, lo, hi)
            assert (i & (P.z == z) & (P.b0 == hi) & (P.b1 == lo) & ~P.sorted).any(), (z, lo, hi)
    ko = kv.key_off.astype(np.int64)
    pl, kl = np.diff(ko)[:-1], np.diff(ko)[1:]
    for m in wc.PREFIX_M:
        full = i & (P.z == P.m) & (P.m == m)
        assert (full & (pl < kl)).any() and (full & (pl > kl) & ~P.sorted).any() and (full & (pl == kl)).any(), m
    assert nun == len(wc.FIRST_DIFF_Z) * len(wc.BYTE_PAIRS) + len(wc.PREFIX_M) + 13
    W = walked(case, pairs=wc.classify_pairs(kv, seg))
    assert sum(b.direct for b in W.blocks) == nun
    print(wc.pairs_line("pair_probes", P))


def test_tail_probes():
    cases = wc.tail_probes()
    assert len(cases) <= 24
    want = {("tail", s, q) for s in (False, True) for q in range(4)}
    for glead in range(16):
        seen, prefix = set(), set()
        for kv, seg, bs in cases:
            P = wc.classify_pairs(kv, seg, 4096 + glead)
            assert P.route[-1] == 2, "the last pair is not on the tail route"
            t = P.route == 2
            seen |= {x for x in P.seen() if x[0] == "tail"}
            ko = kv.key_off.astype(np.int64)
            pl, kl = np.diff(ko)[:-1], np.diff(ko)[1:]
            prefix |= set(np.sign(kl - pl)[t & (P.z == P.m)].tolist())
            uns = (~P.sorted).any()
            assert (~P.sorted[~t]).sum() == 0, "an out-of-order pair off the tail route"
            assert bool(wc.shortcut_differs(kv, P, int(seg[1]), kv.n)) == bool(uns)
        assert want <= seen, f"glead {glead}: missing {sorted(want - seen)}"
        assert prefix == {-1, 0, 1}, "tail route: prefix pairs"
    for case in cases:
        W = walked(case)
        assert len(W.blocks) == 2
    print(wc.pairs_line("tail_probes (last stream)", P))


def test_geometry():
    case = wc.geometry()
    W = walked(case)
    wc.check_geometry(W, case[1])
    print(wc.walk_line("geometry", W))


def test_direct_rewrap():
    case = wc.direct_rewrap()
    kv, seg, bs = case
    P = wc.classify_pairs(kv, seg)
    W = walked(case, pairs=P)
    wc.check_direct_rewrap(W, seg, P)
    print(wc.walk_line("direct_rewrap", W))


@pytest.mark.parametrize("cus", [256, 64])
def test_fused_multi(cus):
    case = wc.fused_multi(cus)
    nwalk, spw = wc.fused_shape(cus, len(case[1]) - 1)
    W = walked(case, ring_base=wc.fused_ring_base(case[1], spw))
    assert wc.check_fused_multi(W, case[1], cus) == (nwalk, spw)
    # the same stream on rings based at every segment (plan_walk_kernel): the same table
    walked(case)
    print(f"{cus} CUs, {nwalk} walkers x {spw} segments; " + wc.walk_line("fused_multi", W))


def test_wide():
    for case in wc.wide():
        W = walked(case, decodes=False)
        wc.check_wide(W, case[2])
        print(wc.walk_line(f"wide {case[2]}", W))


def test_huge():
    cases = wc.huge()
    assert sum(len(c[0].vals) + len(c[0].keys) for c in cases) < 300 << 20
    assert [c[2] for c in cases] == [4096, (1 << 25) + 4096]
    for which, case in enumerate(cases):
        W = walked(case, decodes=False)
        wc.check_huge(W, which)
        print(wc.walk_line(f"huge {which}", W))
