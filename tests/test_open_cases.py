"""CPU: the open rule of open_cases.py agrees with pyref.sst_open, and the generators reach every
window split, residue, edge side and batch shape they were built for.  No GPU, no device call.
The counts are printed (pytest -s shows them) and asserted as equalities: the generators are
constructive."""
import struct
from collections import Counter

import pytest

import get_cases as gc
import open_cases as oc
from oracle import pyref


def pyref_opens_cleanly(buf):
    """pyref.sst_open returns, and what it returns is consistent with the file: every key slice lies
    inside the records, the records fill their section, the offsets are those of framed blocks."""
    try:
        metas, max_ts, bloom, mo = pyref.sst_open(buf)
    except Exception:
        return False
    n = len(buf)
    bo = int.from_bytes(buf[n - 4:], "big")
    if not (20 <= bo <= n - 9 and mo + 16 <= bo - 4 and metas):
        return False
    pos = mo + 4
    for i, (off, fk, lk) in enumerate(metas):
        fl = int.from_bytes(buf[pos + 4:pos + 6], "big")
        ll = int.from_bytes(buf[pos + 6 + fl + 8:pos + 6 + fl + 10], "big")
        pos += 24 + fl + ll
        if len(fk) != fl or len(lk) != ll or pos > bo - 16:  # a slice past the section comes back short
            return False
        if off + 6 > mo or (i and off < metas[i - 1][0] + 6):
            return False
    return pos == bo - 16


def check_rule_equals_pyref(buf):
    err, slots, d, index = oc.open_rule(buf)
    metas, max_ts, bloom, mo = pyref.sst_open(buf)
    assert err == 0 and slots == len(metas) == d["nblk"] == len(index)
    assert d["meta_offset"] == mo and d["max_ts"] == max_ts and d["bloom_k"] == bloom.k
    assert buf[d["bloom_pos"]:d["bloom_pos"] + d["bloom_len"]] == bloom.filter
    assert buf[d["first_key_pos"]:d["first_key_pos"] + d["first_key_len"]] == metas[0][1]
    assert buf[d["last_key_pos"]:d["last_key_pos"] + d["last_key_len"]] == metas[-1][2]
    offs = [m[0] for m in metas]
    assert [r["off"] for r in index] == offs and [r["end"] for r in index] == offs[1:] + [mo]
    assert [buf[r["key_pos"]:r["key_pos"] + r["key_len"]] for r in index] == [m[1] for m in metas]
    assert [(r["img_hi"], r["img_lo"]) for r in index] == [oc.image_ints(m[1]) for m in metas]
    assert all(mo + 4 < r["key_pos"] < d["bloom_pos"] for r in index)


def test_constants_and_the_smallest_file():
    assert oc.kOpenChunk % 1024 == 0 and oc.kMetaRecMin == len(oc.record(0, b"", b"")) == 24
    assert len(oc.smallest_file()) == 59 and oc.open_rule(oc.smallest_file())[:2] == (0, 1)


@pytest.mark.parametrize("name", gc.CASES)
def test_rule_equals_pyref_on_built_files(name):
    for s in gc.case(name).ssts:
        check_rule_equals_pyref(s.buf)


def test_rule_equals_pyref_on_crafted_files():
    files = [b for _, b in oc.long_key_files()] + [oc.healthy(i) for i in range(40)]
    files += [f.buf for k in oc.KINDS for r in (0, 7, 15) for f in oc.straddle_files(k, r)]
    files += [e.buf for e in oc.edge_files() if oc.open_rule(e.buf)[0] == 0]
    for buf in files:
        check_rule_equals_pyref(buf)
        assert pyref_opens_cleanly(buf)
    assert len(files) > 150


def test_no_broken_file_opens_cleanly_in_pyref():
    """Per file: the rule's verdict against pyref.sst_open -- CHECKSUM files raise there, MALFORMED
    files raise or come back inconsistent with the file."""
    verdicts = Counter()
    for label, buf, want in oc.crc_files():
        err = oc.open_rule(buf)[0]
        assert err == want, label
        if err & oc.ERR_CHECKSUM:  # (a record that also runs out of its section ends the decode before the compare)
            with pytest.raises(ValueError if err == oc.ERR_CHECKSUM else (ValueError, struct.error)):
                pyref.sst_open(buf)
        assert pyref_opens_cleanly(buf) == (err == 0), label
        verdicts[err] += 1
    assert verdicts == {0: 2, oc.ERR_CHECKSUM: 7, oc.ERR_CHECKSUM | oc.ERR_MALFORMED: 2}
    clean = Counter()
    for e in oc.edge_files():
        err = oc.open_rule(e.buf)[0]
        assert err in (0, oc.ERR_MALFORMED), e.edge
        assert pyref_opens_cleanly(e.buf) == (err == 0), (e.edge, e.side, len(e.buf))
        clean[err] += 1
    for f in (oc.walk_failed, oc.prep_refused):
        for i in range(3):
            assert not pyref_opens_cleanly(f(i))
    print("edge files: %d open, %d malformed" % (clean[0], clean[oc.ERR_MALFORMED]))


def test_every_window_split_at_every_residue():
    seen = Counter()
    for residue in range(16):
        for kind in oc.KINDS:
            files = oc.straddle_files(kind, residue)
            assert [(f.split, f.fl) for f in files] == oc.SPLITS[kind]
            for f in files:
                assert len(f.buf) % 16 == 0 and oc.open_rule(f.buf)[0] == 0
                n = len(f.buf)
                sect = int.from_bytes(f.buf[n - 4:], "big") - 4 - 40
                assert 2 * oc.kOpenChunk - 64 <= sect <= 3 * oc.kOpenChunk  # two to three windows
                tr = oc.window_trace(f.buf, residue)
                nb = min(f.fl, 16) if kind == "key" else oc.FIELD_BYTES[kind]
                # the construction: record 1's field `split` bytes before the end, record 2's the complement
                last = tr[-1].rec  # 2; 3 where record 1 ended with its window and a short record follows it
                assert last == (3 if (kind, f.split) == ("length", 2) else 2)
                got = [(r.rec, r.before, r.refill) for r in tr if r.kind == kind and r.rec in (1, last)]
                assert got == [(1, f.split, f.split < nb), (last, nb - f.split, f.split > 0)], (kind, residue, f.split, got)
                assert tr[0].first and sum(r.first for r in tr) == 1
                for r in tr:
                    if r.rec:
                        seen[(r.kind, r.nb, r.before, r.refill, residue)] += 1
    for residue in range(16):
        for kind, nb, splits in (("header", 6, range(0, 7)), ("key", 16, range(0, 17)), ("length", 2, range(0, 3))):
            for s in splits:
                assert seen[(kind, nb, s, s < nb, residue)] >= 1, (kind, s, residue)
        # short keys: the staged bytes are the key's own length
        assert all(seen[("key", nb, s, s < nb, residue)] for nb, s in ((1, 0), (1, 1), (7, 3), (7, 7), (7, 4), (7, 0)))
    per_residue = sum(len(v) for v in oc.SPLITS.values())
    assert per_residue == 7 + 23 + 3
    print("straddle files: %d per residue, %d in all; (kind, bytes, split, refill, residue) classes: %d"
          % (per_residue, 16 * per_residue, len(seen)))


def test_long_keys_lie_whole_windows_ahead():
    files = dict(oc.long_key_files())
    assert all(len(b) % 16 == 0 and len(b) <= 300 << 10 and oc.open_rule(b)[0] == 0 for b in files.values())
    gaps = Counter()
    for n in oc.LONG_LENS:
        for which in ("first", "last"):
            buf = files["%s-%d" % (which, n)]
            _, _, d, index = oc.open_rule(buf)
            lens = {r["key_len"] for r in index} | {d["last_key_len"]}
            assert n in lens
            for residue in (0, 9):
                for r in oc.window_trace(buf, residue):
                    gaps[(which, n)] = max(gaps[(which, n)], r.gap // oc.kOpenChunk)
    # the field after a key of n bytes: whole windows between the old window's end and it
    assert all(gaps[(w, n)] >= n // oc.kOpenChunk - 1 for w in ("first", "last") for n in oc.LONG_LENS)
    assert gaps[("first", 3 * oc.kOpenChunk)] >= 2 and gaps[("first", 65535)] >= 6
    _, _, d, index = oc.open_rule(files["both-65535"])
    assert index[0]["key_len"] == 65535 and index[1]["key_pos"] - index[0]["key_pos"] == 2 * 65535 + 24
    assert max(r.gap for r in oc.window_trace(files["both-65535"], 3)) > 6 * oc.kOpenChunk
    assert [r["key_len"] for r in oc.open_rule(files["empty-all"])[3]] == [0, 0, 0]
    assert all((r["img_hi"], r["img_lo"]) == (0, 0) for r in oc.open_rule(files["empty-all"])[3])
    assert not any(r.kind == "key" for r in oc.window_trace(files["empty-all"], 0))
    d = oc.open_rule(files["empty-last"])[2]
    assert d["last_key_len"] == 0 and oc.open_rule(files["empty-first"])[2]["first_key_len"] == 0
    mask = oc.open_rule(files["image-mask"])[3]
    assert [r["key_len"] for r in mask] == [15, 15, 16, 16, 16, 16, 17, 17, 17, 17, 17, 17, 17, 17]
    assert mask[0]["img_lo"] == mask[1]["img_lo"] and mask[0]["img_lo"] & 0xFF == 0   # the ts byte after a 15-byte key
    assert [r["img_lo"] & 0xFF for r in mask[2:6]] == [0, 0, 0xFF, 0xFF]
    assert mask[6]["img_lo"] == mask[8]["img_lo"] != mask[10]["img_lo"] == mask[12]["img_lo"]  # the 17th byte is not in the image
    print("long-key files: %d, largest %d bytes, windows skipped %s"
          % (len(files), max(map(len, files.values())), [gaps[("first", n)] for n in oc.LONG_LENS]))


def test_every_edge_has_both_sides():
    sides, same = Counter(), []
    for e in oc.edge_files():
        sides[(e.edge, e.side)] += 1
    assert {k[0] for k in sides} == set(oc.EDGES)
    assert all(sides[(e, "accept")] >= 1 and sides[(e, "refuse")] >= 1 for e in oc.EDGES)
    for edge in oc.EDGES:
        res = {side: {oc.open_rule(e.buf)[:2] for e in oc.edge_files() if e.edge == edge and e.side == side}
               for side in ("accept", "refuse")}
        assert all(err == oc.ERR_MALFORMED for err, _ in res["refuse"]), edge
        if any(err for err, _ in res["accept"]):
            same.append(edge)
            assert res["accept"] == res["refuse"] == {(oc.ERR_MALFORMED, 0)}
    assert tuple(same) == oc.SAME_BOTH_SIDES
    # both kinds of failure: refused by the prep checks (no slot), failed in the walk (slots stay reserved)
    kinds = Counter((e.edge, oc.open_rule(e.buf)[1] > 0) for e in oc.edge_files() if e.side == "refuse")
    prep = ("bloom_offset_low", "bloom_offset_high", "meta_offset_high", "num_low", "num_section", "file_length")
    assert all((kinds[(e, True)] == 0) == (e in prep) and (kinds[(e, False)] == 0) == (e not in prep) for e in oc.EDGES)
    assert sides[("file_length", "refuse")] == 3 * 59 and sides[("file_length", "accept")] == 1
    lens = Counter(len(e.buf) for e in oc.edge_files() if e.edge == "file_length" and e.side == "refuse")
    assert lens == {n: 3 for n in range(59)}
    print("edges: %d, files per (edge, side): %s; indistinguishable sides: %s" % (len(oc.EDGES), dict(sides), same))


def test_every_batch_shape_is_present():
    shapes = {b.name: oc.batch_shape(b) for b in oc.batches()}
    assert sorted({s["n"] for s in shapes.values()}) == [1, 2, 3, 65, 130]
    live = [s for s in shapes.values() if not s["decreasing"]]
    assert sum(s["decreasing"] for s in shapes.values()) == 1
    for kind in ("reserved", "none"):
        assert set().union(*(s[kind] for s in live)) == {"first", "middle", "last"}, kind
    assert sum(s["neighbours"] for s in live) == 2 and sum(s["zero_between"] for s in live) == 1
    one = [b for b in oc.batches() if len(b.bufs) == 1]
    assert sorted(oc.open_rule(b.bufs[0])[:2] for b in one) == [(0, 1), (oc.ERR_MALFORMED, 0), (oc.ERR_MALFORMED, 3)]
    for b in oc.batches():
        blob, off = oc.batch_layout(b)
        r = oc.open_batch_rule(blob, off)
        if shapes[b.name]["decreasing"]:
            assert r["stats"][0] == 0 and r["stats"][3] == oc.ERR_MALFORMED
            continue
        assert off[-1] == len(blob) <= 300 << 10 and len(b.bufs) <= 130
        assert r["stats"][0] == sum(d["err"] == 0 for d in r["desc"]) and r["stats"][1] == len(r["index"])
        assert r["stats"][1] > sum(d["nblk"] for d in r["desc"]) or not any(oc.open_rule(x)[0] and oc.open_rule(x)[1] for x in b.bufs)
        # a later SST's blk0 counts the slots of the walk-failed SSTs before it, not those of the refused
        assert [d["blk0"] for d in r["desc"]] == [sum(oc.open_rule(x)[1] for x in b.bufs[:s]) for s in range(len(b.bufs))]
        short = oc.open_batch_rule(blob, off, r["reserved"] - 1) if r["reserved"] else None
        assert short is None or short["stats"] == [0, r["reserved"], None, oc.ERR_CAPACITY]
    print("batches: %s" % {k: (v["n"], sorted(v.get("reserved", ())), sorted(v.get("none", ()))) for k, v in shapes.items()})
