"""Range scans over an LSM view on the device (lsmblk_lsm_scan_batch; lsm_amd.sst.SstSet.lsm_scan*)
against the CPU expectations of lsm_scan_cases.py: every result field, seg_start, the eight stats
words and every byte of the out and raw streams in the three modes, the capacity contract of
sub_cap / raw / out, the view check's and the ranges' error reports, workspace regrowth on a
non-default stream, and the composition the call replaces (scan -> merge per range -> read filter)."""
import numpy as np
import pytest
import torch

import lsm_get_cases as lc
import lsm_scan_cases as ls
import scan_cases as sc
from gpu_kit import (GUARD, _need_gpu, all_empty, check_results, check_stream,  # noqa: F401 (_need_gpu: autouse)
                     guarded, opened_view, sizes_of, untouched)
from lsm_amd import batch, sst
from lsm_amd._lib import (LSMBLK_ERR_CAPACITY, LSMBLK_ERR_EMPTY_KEY, LSMBLK_ERR_MALFORMED, LSMBLK_ERR_SEGMENTS,
                          LSMBLK_E_INVAL, LSMBLK_SCAN_NO_FILTER, LsmBlkError)

pytestmark = pytest.mark.gpu


def opened(name, bs):
    """(the case, its SstSet, its view)"""
    c = ls.case(name, bs)
    return (c, *opened_view(c.view, ("lsm_scan", name, bs)))


def flags_of(mode):
    return 2 if ls.mode_args(mode)[0] else 0


def run(ss, view, c, sel, mode, raw_caps, out_caps, **kw):
    pick = lambda x: [x[i] for i in sel]
    ts = pick(c.read_ts) if ls.mode_args(mode)[1] else None
    return ss.lsm_scan_raw(view, pick(c.lower), pick(c.upper), pick(c.lkind), pick(c.ukind), ts, flags_of(mode),
                           raw_caps=raw_caps, out_caps=out_caps, **kw)


@pytest.mark.parametrize("mode", ls.MODES)
@pytest.mark.parametrize("name,bs", ls.CASES)
def test_every_field_and_byte_equals_the_expectation(name, bs, mode):
    c, ss, view = opened(name, bs)
    exp, out_rows, raw_runs = ls.expected(name, bs, mode)
    n, kb, vb = sizes_of(out_rows)
    rn, rkb, rvb = sizes_of(raw_runs)
    r, seg, raw, out, st = run(ss, view, c, range(len(c)), mode, (rn, rkb, rvb), (n, kb, vb))  # exact capacities
    assert st == [n, kb, vb, 0, rn, rkb, rvb, len(raw_runs)]
    check_results(r, exp, ls.FIELDS)
    check_stream(out, out_rows, seg)
    check_stream(raw, raw_runs)
    if mode == "merged":
        assert (r["n"] == r["merged"]).all()
    if (name, bs) in (("owners", 128), ("levels", 128)):  # the wrapper: its own sizes, one retry at the most
        mvcc, filt = ls.mode_args(mode)
        res, got = ss.lsm_scan(view, c.lower, c.upper, lower_kind=c.lkind, upper_kind=c.ukind,
                               read_ts=c.read_ts if filt else None, mvcc=mvcc)
        assert got == out_rows and all((res[f].astype(np.uint64) == exp[f]).all() for f in ls.FIELDS)


@pytest.mark.parametrize("nq", ls.query_counts())
def test_query_counts(nq):
    c, ss, view = opened("owners", 128)
    sel = [(7 * i) % len(c) for i in range(nq)]
    rws = [ls.rows("owners", 128, "mvcc")[i] for i in sel]
    exp, out_rows, raw_runs = ls.arrays(rws)
    r, seg, raw, out, st = run(ss, view, c, sel, "mvcc", sizes_of(raw_runs), sizes_of(out_rows))
    assert st == [*sizes_of(out_rows), 0, *sizes_of(raw_runs), len(raw_runs)]
    check_results(r, exp, ls.FIELDS)
    check_stream(out, out_rows, seg)
    check_stream(raw, raw_runs)


def test_sizing_calls_and_the_capacity_contract():
    c, ss, view = opened("owners", 128)
    exp, out_rows, raw_runs = ls.expected("owners", 128, "default")
    (n, kb, vb), (rn, rkb, rvb), subs, nq = sizes_of(out_rows), sizes_of(raw_runs), len(raw_runs), len(c)
    want_seg = sc.stream_of(out_rows)[5].tolist()
    full = [n, kb, vb, 0, rn, rkb, rvb, subs]
    dev, sel = ss.device, range(nq)
    assert min(n, kb, vb, subs) > 1
    # no stream at all: the table scans' sizes
    r, seg, _, _, st = run(ss, view, c, sel, "default", None, None)
    assert st == [0, 0, 0, 0, rn, rkb, rvb, subs] and seg.tolist() == [0] * (nq + 1)
    check_results(r, exp, ("sources", "raw"))
    assert (r["merged"] == 0).all() and (r["n"] == 0).all()
    # out = NULL: every size, res and seg_start
    r, seg, raw, out, st = run(ss, view, c, sel, "default", (rn, rkb, rvb), None)
    assert out is None and st == full and seg.tolist() == want_seg
    check_results(r, exp, ls.FIELDS)
    check_stream(raw, raw_runs)
    # sub_cap one short: no scan runs
    raw, out = guarded(rn, rkb, rvb, dev), guarded(n, kb, vb, dev)
    r, seg, _, _, st = run(ss, view, c, sel, "default", (rn, rkb, rvb), (n, kb, vb), sub_cap=subs - 1, raw=raw, out=out)
    assert st[3] == LSMBLK_ERR_CAPACITY and st[7] == subs
    all_empty(r, seg, nq)
    assert untouched(raw, offsets=False) and untouched(out, offsets=False)
    # a capacity of raw one short
    for short in range(3):
        caps = [rn, rkb, rvb]
        caps[short] -= 1
        raw, out = guarded(rn, rkb, rvb, dev), guarded(n, kb, vb, dev)
        r, seg, _, _, st = run(ss, view, c, sel, "default", tuple(caps), (n, kb, vb), raw=raw, out=out)
        assert st == [0, 0, 0, LSMBLK_ERR_CAPACITY, rn, rkb, rvb, subs] and seg.tolist() == [0] * (nq + 1), short
        check_results(r, exp, ("sources", "raw"))
        assert (r["merged"] == 0).all() and (r["n"] == 0).all() and (r["status"] == ls.EMPTY).all()
        assert untouched(raw), short
    # a capacity of out one short
    for short in range(3):
        caps = [n, kb, vb]
        caps[short] -= 1
        raw, out = guarded(rn, rkb, rvb, dev), guarded(n, kb, vb, dev)
        r, seg, raw, _, st = run(ss, view, c, sel, "default", (rn, rkb, rvb), tuple(caps), raw=raw, out=out)
        assert st == [n, kb, vb, LSMBLK_ERR_CAPACITY, rn, rkb, rvb, subs] and seg.tolist() == want_seg, short
        check_results(r, exp, ls.FIELDS)
        assert untouched(out), short
        raw.n = rn
        check_stream(raw, raw_runs)
    # exactly enough: the guard bytes after the arenas stay
    raw, out = guarded(rn, rkb, rvb, dev), guarded(n, kb, vb, dev)
    r, seg, raw, out, st = run(ss, view, c, sel, "default", (rn, rkb, rvb), (n, kb, vb), sub_cap=subs, raw=raw, out=out)
    assert st == full
    check_stream(out, out_rows, seg)
    check_stream(raw, raw_runs)
    assert (out.keys[kb:] == GUARD).all() and (out.vals[vb:] == GUARD).all()
    assert (raw.keys[rkb:] == GUARD).all() and (raw.vals[rvb:] == GUARD).all()


# ------------------------------------------------------------------------------ the view check
def refused(ss, view, c, flag):
    nq = 40
    for mode in ls.MODES:
        r, seg, raw, out, st = run(ss, view, c, range(nq), mode, (4096, 65536, 65536), (4096, 65536, 65536))
        assert st == [0, 0, 0, flag, 0, 0, 0, 0], mode
        all_empty(r, seg, nq)
    with pytest.raises(LsmBlkError):
        ss.lsm_scan(view, c.lower[:nq], c.upper[:nq], lower_kind=c.lkind[:nq], upper_kind=c.ukind[:nq], read_ts=5)


def test_view_with_an_id_past_the_set():
    c, ss, _ = opened("mixed", 128)
    v = c.view
    refused(ss, ss.view(v.l0 + [ss.nsst], v.levels), c, LSMBLK_ERR_SEGMENTS)


def test_view_with_a_decreasing_level_start():
    c, ss, _ = opened("mixed", 128)
    view = ss.view(c.view.l0, c.view.levels)
    view.level_start_t = batch._u32_table(np.array([0, 5, 3], np.uint32), ss.device)
    refused(ss, view, c, LSMBLK_ERR_SEGMENTS)


def test_view_with_overlapping_neighbours():
    c, ss, _ = opened("mixed", 128)
    v = c.view
    x, y = sorted(v.l0[:2], key=lambda t: lc.first_key(v.ssts[t]))
    assert lc.first_key(v.ssts[x]) < lc.first_key(v.ssts[y]) <= lc.last_key(v.ssts[x])
    refused(ss, ss.view([v.l0[2]], [v.levels[0], [x, y]]), c, LSMBLK_ERR_MALFORMED)


# ------------------------------------------------------------------------------ bad ranges
def with_one_bad_range(flag, lk, lo, uk, up):
    """Range 5 of the first 30 replaced: it is empty with no source, the flag is raised, the others answer."""
    c, ss, view = opened("mixed", 128)
    exp, out_rows, _ = ls.expected("mixed", 128, "default")
    nq, bad = 30, 5
    lower, upper, lkind, ukind = list(c.lower[:nq]), list(c.upper[:nq]), list(c.lkind[:nq]), list(c.ukind[:nq])
    lower[bad], upper[bad], lkind[bad], ukind[bad] = lo, up, lk, uk
    r, seg, _, out, st = ss.lsm_scan_raw(view, lower, upper, lkind, ukind, c.read_ts[:nq], 0, raw_caps=(4096, 65536, 65536),
                                         out_caps=(4096, 65536, 65536))
    assert st[3] == flag
    rows = [[] if i == bad else out_rows[i] for i in range(nq)]
    check_stream(out, rows, seg)
    assert r["status"][bad] == ls.EMPTY and all(r[f][bad] == 0 for f in ("sources", "raw", "merged", "n"))
    ok = np.arange(nq) != bad
    for f in ls.FIELDS:
        assert (r[f][ok].astype(np.uint64) == exp[f][:nq][ok]).all(), f


def test_a_bound_kind_of_3():
    with_one_bad_range(LSMBLK_ERR_SEGMENTS, 3, b"a", sc.INCLUDED, b"b")
    with_one_bad_range(LSMBLK_ERR_SEGMENTS, sc.UNBOUNDED, b"", 3, b"b")


def test_an_empty_bounded_key():
    with_one_bad_range(LSMBLK_ERR_EMPTY_KEY, sc.INCLUDED, b"", sc.UNBOUNDED, b"")
    with_one_bad_range(LSMBLK_ERR_EMPTY_KEY, sc.INCLUDED, b"a", sc.EXCLUDED, b"")


def test_a_malformed_block_empties_its_ranges_only():
    """A block of an L0 table breaks the decode rules: every range whose scan of that table visits it
    is empty with zero counts -- never a partial merge -- MALFORMED is raised, the others are unchanged."""
    c = ls.case("mixed", 128)
    v = c.view
    t = v.l0[2]
    s = v.ssts[t]
    victim = len(s.blocks) // 2
    bufs = [ls.corrupt_block(x, victim) if i == t else x.buf for i, x in enumerate(v.ssts)]
    ss = sst.SstSet(b"".join(bufs), v.file_off)
    view = ss.view(v.l0, v.levels)
    rws = ls.rows("mixed", 128, "mvcc")
    # clean: the table is not scanned, or neither bound is searched near the victim and the range ends before / begins after it
    lo_k, hi_k = s.blocks[victim - 2][0][0], s.blocks[victim + 2][-1][0]
    far = lambda k: not k or k < lo_k or k > hi_k
    clean = [i for i, (lk, lo, uk, up, _) in enumerate(c.ranges())
             if not ls.passes(s, lk, lo, uk, up) or (lk and uk and far(lo) and far(up) and (up < lo_k or lo > hi_k))]
    assert len(clean) >= 20
    dirty = [(sc.INCLUDED, s.blocks[victim - 1][0][0], sc.INCLUDED, s.blocks[victim + 1][-1][0]),
             (sc.EXCLUDED, s.blocks[victim - 1][-1][0], sc.UNBOUNDED, b""),
             (sc.UNBOUNDED, b"", sc.EXCLUDED, s.blocks[victim + 1][0][0])]
    pick = lambda x: [x[i] for i in clean]
    lower = pick(c.lower) + [d[1] for d in dirty]
    upper = pick(c.upper) + [d[3] for d in dirty]
    lkind = pick(c.lkind) + [d[0] for d in dirty]
    ukind = pick(c.ukind) + [d[2] for d in dirty]
    ts = pick(c.read_ts) + [ls.TS_MAX] * len(dirty)
    r, seg, _, out, st = ss.lsm_scan_raw(view, lower, upper, lkind, ukind, ts, 2, raw_caps=(20000, 400000, 800000),
                                         out_caps=(20000, 400000, 800000))
    assert st[3] == LSMBLK_ERR_MALFORMED
    exp, out_rows, _ = ls.arrays([rws[i] for i in clean])
    check_results(r[:len(clean)], exp, ls.FIELDS)
    check_stream(out, out_rows + [[] for _ in dirty], seg)
    tail = r[len(clean):]
    assert (tail["status"] == ls.EMPTY).all() and all((tail[f] == 0).all() for f in ("sources", "raw", "merged", "n"))


def test_no_filter_is_refused_and_an_empty_batch_is_answered():
    c, ss, view = opened("mixed", 128)
    with pytest.raises(LsmBlkError) as e:
        ss.lsm_scan_raw(view, c.lower[:4], c.upper[:4], c.lkind[:4], c.ukind[:4], 7, LSMBLK_SCAN_NO_FILTER,
                        raw_caps=(64, 1024, 1024), out_caps=(64, 1024, 1024))
    assert e.value.status == LSMBLK_E_INVAL
    with pytest.raises(LsmBlkError) as e:  # out without raw
        ss.lsm_scan_raw(view, c.lower[:4], c.upper[:4], c.lkind[:4], c.ukind[:4], 7, 0, out_caps=(64, 1024, 1024))
    assert e.value.status == LSMBLK_E_INVAL
    raw, out = guarded(4, 64, 64, ss.device), guarded(4, 64, 64, ss.device)
    r, seg, _, _, st = ss.lsm_scan_raw(view, [], [], [], [], [], 0, raw_caps=(4, 64, 64), out_caps=(4, 64, 64), raw=raw, out=out)
    assert st == [0] * 8 and len(r) == 0 and seg.tolist() == [0]
    for kv in (raw, out):
        assert kv.key_off[0].item() == 0 and kv.val_off[0].item() == 0 and (kv.key_off[1:] == -1).all()
    res, rows = ss.lsm_scan(view, [], [], lower_kind=[], upper_kind=[], read_ts=3)
    assert rows == [] and len(res["n"]) == 0


def test_workspace_regrowth_on_a_non_default_stream():
    """A fresh stream has a fresh context: a small call, then a larger one that regrows its workspace."""
    c = ls.case("levels", 128)
    exp, out_rows, raw_runs = ls.expected("levels", 128, "default")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        ss = sst.SstSet(c.view.files, c.view.file_off, stream=stream)
        view = ss.view(c.view.l0, c.view.levels)
        small = list(range(4, 9))
        rws = [ls.rows("levels", 128, "default")[i] for i in small]
        e1, o1, r1 = ls.arrays(rws)
        r, seg, raw, out, st = run(ss, view, c, small, "default", sizes_of(r1), sizes_of(o1))
        assert st[3] == 0
        check_results(r, e1, ls.FIELDS)
        check_stream(out, o1, seg)
        r, seg, raw, out, st = run(ss, view, c, range(len(c)), "default", sizes_of(raw_runs), sizes_of(out_rows))
        assert st == [*sizes_of(out_rows), 0, *sizes_of(raw_runs), len(raw_runs)]
        check_results(r, exp, ls.FIELDS)
        check_stream(out, out_rows, seg)
        check_stream(raw, raw_runs)
    torch.cuda.synchronize()


@pytest.mark.parametrize("mvcc", (False, True))
def test_agrees_with_scan_merge_and_read_filter_per_range(mvcc):
    """The composition the call replaces, over a view of 10 tables: the tables expanded on the host,
    one SstSet.scan_raw over them, one merge per range, the read filter -- byte for byte."""
    c, ss, view = opened("mixed", 256)
    v = c.view
    sel = list(range(0, len(c), 2))  # (a range's three read_ts values follow each other: a stride of 2 takes all three)
    pick = lambda x: [x[i] for i in sel]
    _, got = ss.lsm_scan(view, pick(c.lower), pick(c.upper), lower_kind=pick(c.lkind), upper_kind=pick(c.ukind),
                         read_ts=pick(c.read_ts), mvcc=mvcc)
    nonempty = 0
    for j, i in enumerate(sel):
        lk, lo, uk, up, ts = c.lkind[i], c.lower[i], c.ukind[i], c.upper[i], c.read_ts[i]
        tabs = [t for t in ls.tables(v) if sc.range_overlap(lk, lo, uk, up, ss.first_key(t), ss.last_key(t))]
        if not tabs:
            assert got[j] == []
            continue
        r, seg, kv, st = ss.scan_raw(tabs, [lo] * len(tabs), [up] * len(tabs), lk, uk, 2 if mvcc else 0, (4096, 65536, 131072))
        assert st[3] == 0
        if kv.n == 0:
            assert got[j] == []
            continue
        m = batch.merge_runs(kv, seg)
        f, fseg = batch.read_filter(m, [0, m.n], ts)
        keys, ko, vals, vo, fts = f.to_numpy()
        kb, vb = keys.tobytes(), vals.tobytes()
        assert got[j] == [(kb[ko[x]:ko[x + 1]], int(fts[x]), vb[vo[x]:vo[x + 1]]) for x in range(f.n)], i
        nonempty += bool(got[j])
    assert nonempty >= 10
