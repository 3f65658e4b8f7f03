"""Snapshot range scans over an LSM view on the device (lsmblk_lsm_scan_batch with
LSMBLK_LSM_SCAN_NEWEST; lsm_amd.sst.SstSet.lsm_scan(newest=True)) against the CPU expectations of
lsm_scan_newest_cases.py: every result field, seg_start, the eight stats words and every byte of the
out and raw streams with and without q_ts, the composition with lsmblk_read_filter_batch, agreement
with the NEWEST point read, the capacity contract, the flag bits and a malformed block."""
import numpy as np
import pytest

import lsm_scan_cases as ls
import lsm_scan_newest_cases as ln
import scan_cases as sc
from gpu_kit import (GUARD, _need_gpu, all_empty, check_results, check_stream,  # noqa: F401 (_need_gpu: autouse)
                     guarded, opened_view, sizes_of, untouched)
from lsm_amd import batch, sst
from lsm_amd._lib import (LSMBLK_ERR_CAPACITY, LSMBLK_ERR_MALFORMED, LSMBLK_E_INVAL, LSMBLK_GET_FOUND,
                          LSMBLK_LSM_SCAN_NEWEST, LSMBLK_SCAN_MVCC, LSMBLK_SCAN_NO_FILTER, LsmBlkError)

pytestmark = pytest.mark.gpu

NEWEST = LSMBLK_LSM_SCAN_NEWEST


def opened(name, bs):
    """(the case, its SstSet, its view)"""
    c = ln.case(name, bs)
    return (c, *opened_view(c.view, ("lsm_scan_newest", name, bs)))


def run(ss, view, c, sel, mode, raw_caps, out_caps, flags=NEWEST, **kw):
    pick = lambda x: [x[i] for i in sel]
    ts = pick(c.read_ts) if mode == "view" else None
    return ss.lsm_scan_raw(view, pick(c.lower), pick(c.upper), pick(c.lkind), pick(c.ukind), ts, flags, raw_caps=raw_caps,
                           out_caps=out_caps, **kw)


def same_stream(a, b):
    assert a.n == b.n
    for x, y in zip(a.to_numpy(), b.to_numpy()):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("mode", ln.MODES)
@pytest.mark.parametrize("name,bs", ln.CASES)
def test_every_field_and_byte_equals_the_expectation(name, bs, mode):
    c, ss, view = opened(name, bs)
    exp, out_rows, raw_runs = ln.expected(name, bs, mode)
    n, kb, vb = sizes_of(out_rows)
    rn, rkb, rvb = sizes_of(raw_runs)
    r, seg, raw, out, st = run(ss, view, c, range(len(c)), mode, (rn, rkb, rvb), (n, kb, vb))  # exact capacities
    assert st == [n, kb, vb, 0, rn, rkb, rvb, len(raw_runs)]
    check_results(r, exp, ln.FIELDS)
    check_stream(out, out_rows, seg)
    check_stream(raw, raw_runs)
    assert (r["merged"] == r["raw"]).all()
    if mode == "merged":
        assert (r["n"] == r["merged"]).all()
    if (name, bs) in (("versions", 128), ("levels", 128)):  # the wrapper: its own sizes, one retry at the most
        res, got = ss.lsm_scan(view, c.lower, c.upper, lower_kind=c.lkind, upper_kind=c.ukind,
                               read_ts=c.read_ts if mode == "view" else None, newest=True)
        assert got == out_rows and all((res[f].astype(np.uint64) == exp[f]).all() for f in ln.FIELDS)


@pytest.mark.parametrize("name,bs", (("versions", 128), ("owners", 128), ("levels", 128)))
def test_the_read_filter_over_the_merged_stream_equals_the_view(name, bs):
    """lsmblk_read_filter_batch over the q_ts = NULL output, by its seg_start and the ranges' read_ts,
    is the q_ts output byte for byte."""
    c, ss, view = opened(name, bs)
    _, out_rows, raw_runs = ln.expected(name, bs, "view")
    caps = sizes_of(raw_runs)
    _, mseg, _, merged, st = run(ss, view, c, range(len(c)), "merged", caps, caps)
    assert st[3] == 0 and merged.n == caps[0] > 0
    _, seg, _, out, st = run(ss, view, c, range(len(c)), "view", caps, sizes_of(out_rows))
    assert st[3] == 0
    f, fseg = batch.read_filter(merged, mseg, np.array(c.read_ts, np.uint64))
    assert fseg.tolist() == seg.tolist()
    same_stream(f, out)


@pytest.mark.parametrize("name,bs", (("versions", 128), ("owners", 128)))
def test_point_ranges_agree_with_the_newest_point_read(name, bs):
    c, ss, view = opened(name, bs)
    idx = ln.point_ranges(name, bs)
    keys, ts = [c.lower[i] for i in idx], [c.read_ts[i] for i in idx]
    _, rows = ss.lsm_scan(view, keys, keys, lower_kind=[sc.INCLUDED] * len(idx), upper_kind=[sc.INCLUDED] * len(idx),
                          read_ts=ts, newest=True)
    g = ss.lsm_get(view, keys, ts, newest=True)
    found = 0
    for j in range(len(idx)):
        if g["status"][j] == LSMBLK_GET_FOUND:
            assert rows[j] == [(keys[j], int(g["ts"][j]), g["values"][j])], (j, keys[j], ts[j])
            found += 1
        else:
            assert rows[j] == [], (j, keys[j], ts[j])
    assert 10 <= found < len(idx)


def test_sizing_calls_and_the_capacity_contract():
    c, ss, view = opened("versions", 128)
    exp, out_rows, raw_runs = ln.expected("versions", 128, "view")
    (n, kb, vb), (rn, rkb, rvb), subs, nq = sizes_of(out_rows), sizes_of(raw_runs), len(raw_runs), len(c)
    want_seg = sc.stream_of(out_rows)[5].tolist()
    full = [n, kb, vb, 0, rn, rkb, rvb, subs]
    dev, sel = ss.device, range(nq)
    assert min(n, kb, vb, subs) > 1
    # no stream at all: the table scans' sizes
    r, seg, _, _, st = run(ss, view, c, sel, "view", None, None)
    assert st == [0, 0, 0, 0, rn, rkb, rvb, subs] and seg.tolist() == [0] * (nq + 1)
    check_results(r, exp, ("sources", "raw"))
    assert (r["merged"] == 0).all() and (r["n"] == 0).all()
    # out = NULL: every size, res and seg_start
    r, seg, raw, out, st = run(ss, view, c, sel, "view", (rn, rkb, rvb), None)
    assert out is None and st == full and seg.tolist() == want_seg
    check_results(r, exp, ln.FIELDS)
    check_stream(raw, raw_runs)
    # sub_cap one short: no scan runs
    raw, out = guarded(rn, rkb, rvb, dev), guarded(n, kb, vb, dev)
    r, seg, _, _, st = run(ss, view, c, sel, "view", (rn, rkb, rvb), (n, kb, vb), sub_cap=subs - 1, raw=raw, out=out)
    assert st[3] == LSMBLK_ERR_CAPACITY and st[7] == subs
    all_empty(r, seg, nq)
    assert untouched(raw, offsets=False) and untouched(out, offsets=False)
    # a capacity of raw one short
    for short in range(3):
        caps = [rn, rkb, rvb]
        caps[short] -= 1
        raw, out = guarded(rn, rkb, rvb, dev), guarded(n, kb, vb, dev)
        r, seg, _, _, st = run(ss, view, c, sel, "view", tuple(caps), (n, kb, vb), raw=raw, out=out)
        assert st == [0, 0, 0, LSMBLK_ERR_CAPACITY, rn, rkb, rvb, subs] and seg.tolist() == [0] * (nq + 1), short
        check_results(r, exp, ("sources", "raw"))
        assert (r["merged"] == 0).all() and (r["n"] == 0).all() and (r["status"] == ln.EMPTY).all()
        assert untouched(raw), short
    # a capacity of out one short
    for short in range(3):
        caps = [n, kb, vb]
        caps[short] -= 1
        raw, out = guarded(rn, rkb, rvb, dev), guarded(n, kb, vb, dev)
        r, seg, raw, _, st = run(ss, view, c, sel, "view", (rn, rkb, rvb), tuple(caps), raw=raw, out=out)
        assert st == [n, kb, vb, LSMBLK_ERR_CAPACITY, rn, rkb, rvb, subs] and seg.tolist() == want_seg, short
        check_results(r, exp, ln.FIELDS)
        assert untouched(out), short
        raw.n = rn
        check_stream(raw, raw_runs)
    # exactly enough: the guard bytes after the arenas stay
    raw, out = guarded(rn, rkb, rvb, dev), guarded(n, kb, vb, dev)
    r, seg, raw, out, st = run(ss, view, c, sel, "view", (rn, rkb, rvb), (n, kb, vb), sub_cap=subs, raw=raw, out=out)
    assert st == full
    check_stream(out, out_rows, seg)
    check_stream(raw, raw_runs)
    assert (out.keys[kb:] == GUARD).all() and (out.vals[vb:] == GUARD).all()
    assert (raw.keys[rkb:] == GUARD).all() and (raw.vals[rvb:] == GUARD).all()
    # an empty batch
    raw, out = guarded(4, 64, 64, dev), guarded(4, 64, 64, dev)
    r, seg, _, _, st = ss.lsm_scan_raw(view, [], [], [], [], [], NEWEST, raw_caps=(4, 64, 64), out_caps=(4, 64, 64), raw=raw, out=out)
    assert st == [0] * 8 and len(r) == 0 and seg.tolist() == [0]
    for kv in (raw, out):
        assert kv.key_off[0].item() == 0 and kv.val_off[0].item() == 0 and (kv.key_off[1:] == -1).all()
    res, rows = ss.lsm_scan(view, [], [], lower_kind=[], upper_kind=[], read_ts=3, newest=True)
    assert rows == [] and len(res["n"]) == 0


def test_the_flag_bits():
    c, ss, view = opened("versions", 128)
    for flags in (NEWEST | LSMBLK_SCAN_NO_FILTER, NEWEST | 8, NEWEST | LSMBLK_SCAN_MVCC | LSMBLK_SCAN_NO_FILTER, NEWEST | 16):
        with pytest.raises(LsmBlkError) as e:
            ss.lsm_scan_raw(view, c.lower[:4], c.upper[:4], c.lkind[:4], c.ukind[:4], 7, flags, raw_caps=(64, 1024, 1024),
                            out_caps=(64, 1024, 1024))
        assert e.value.status == LSMBLK_E_INVAL, flags
    for mode in ln.MODES:  # NEWEST | MVCC is NEWEST, byte for byte
        _, out_rows, raw_runs = ln.expected("versions", 128, mode)
        caps = sizes_of(raw_runs), sizes_of(out_rows)
        a = run(ss, view, c, range(len(c)), mode, *caps)
        b = run(ss, view, c, range(len(c)), mode, *caps, flags=NEWEST | LSMBLK_SCAN_MVCC)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist() and a[4] == b[4] and a[4][3] == 0
        same_stream(a[2], b[2])
        same_stream(a[3], b[3])
        check_stream(b[3], out_rows, b[1])


def test_a_malformed_block_empties_its_ranges_only():
    """A block in the middle of m-many's versions breaks the decode rules: every range that takes the
    key is empty with zero counts -- never a partial merge -- MALFORMED is raised, the others are
    unchanged."""
    c = ln.case("versions", 128)
    v = c.view
    t = v.levels[1][0]
    s = v.ssts[t]
    many = ln.T + b"m-many"
    stretch = [b for b, blk in enumerate(s.blocks) if all(e[0] == many for e in blk)]
    assert len(stretch) >= 9
    victim = stretch[len(stretch) // 2]
    bufs = [ls.corrupt_block(x, victim) if i == t else x.buf for i, x in enumerate(v.ssts)]
    ss = sst.SstSet(b"".join(bufs), v.file_off)
    view = ss.view(v.l0, v.levels)
    rws = ln.rows("versions", 128, "view")
    # clean: neither bound is searched inside the stretch (no bound begins with "m") and the range does not take the key
    far = lambda k: not k.startswith(ln.T + b"m")
    clean = [i for i, (lk, lo, uk, up, _) in enumerate(c.ranges())
             if far(lo) and far(up) and (not lo or not up or lo <= up) and not ln.in_bounds(many, lk, lo, uk, up)]
    dirty = [i for i, (lk, lo, uk, up, _) in enumerate(c.ranges()) if lo != up and ln.in_bounds(many, lk, lo, uk, up)][:6]
    dirty += [i for i in ln.point_ranges("versions", 128) if c.lower[i] == many][:3]
    assert len(clean) >= 40 and len(dirty) >= 6
    assert sum(rws[i]["n"] for i in clean) > 100 and all(rws[i]["raw"] > 0 for i in dirty)
    sel = clean + dirty
    r, seg, _, out, st = run(ss, view, c, sel, "view", (20000, 800000, 400000), (20000, 800000, 400000))
    assert st[3] == LSMBLK_ERR_MALFORMED
    exp, out_rows, _ = ls.arrays([rws[i] for i in clean])
    check_results(r[:len(clean)], exp, ln.FIELDS)
    check_stream(out, out_rows + [[] for _ in dirty], seg)
    tail = r[len(clean):]
    assert (tail["status"] == ln.EMPTY).all() and all((tail[f] == 0).all() for f in ("sources", "raw", "merged", "n"))
