"""Batched SST range scans and the read-ts visibility filter on the device (lsmblk_sst_scan_batch,
lsmblk_read_filter_batch; lsm_amd.sst.SstSet.scan*, lsm_amd.batch.read_filter) against the CPU
restatements of scan_cases.py: every field of every result, seg_start, the stats and every output
byte in all four flag combinations, the capacity contract, placements, and the composition
scan -> merge -> read filter against LsmIterator over MergeIterator."""
import ctypes

import numpy as np
import pytest
import torch

import get_cases as gc
import scan_cases as sc
from gpu_kit import (GUARD, _need_gpu, check_results, check_stream, guarded, opened_set, sizes_of, untouched)  # noqa: F401 (_need_gpu: autouse)
from lsm_amd import batch, sst
from lsm_amd._lib import (LSMBLK_DEBUG_SCAN_UNITS, LSMBLK_ERR_CAPACITY, LSMBLK_ERR_EMPTY_KEY, LSMBLK_ERR_MALFORMED,
                          LSMBLK_ERR_SEGMENTS, LsmBlkError, ScanResultC, lib)
from oracle import pyref

pytestmark = pytest.mark.gpu


def opened(name):
    return opened_set(sc.case(name), ("scan", name))


def flags_of(no_filter, mvcc):
    return (1 if no_filter else 0) | (2 if mvcc else 0)


def run(ss, c, sel, flags, caps):
    pick = lambda x: [x[i] for i in sel]
    return ss.scan_raw(pick(c.q_sst), pick(c.lower), pick(c.upper), pick(c.lkind), pick(c.ukind), flags, caps)


@pytest.mark.parametrize("no_filter,mvcc", sc.MODES)
@pytest.mark.parametrize("name", sc.CASES)
def test_scan_equals_expectation(name, no_filter, mvcc):
    c, ss = sc.case(name), opened(name)
    exp, rows = sc.expected(name, no_filter, mvcc)
    n, kb, vb = sizes_of(rows)
    r, seg, kv, st = run(ss, c, range(len(c)), flags_of(no_filter, mvcc), (n, kb, vb))
    assert st == [n, kb, vb, 0]
    check_results(r, exp, sc.FIELDS)
    check_stream(kv, rows, seg)


@pytest.mark.parametrize("name", ("bs256", "threshold"))
def test_sizing_call_and_capacity_contract(name):
    c, ss = sc.case(name), opened(name)
    exp, rows = sc.expected(name, False, False)
    n, kb, vb = sizes_of(rows)
    want_seg = sc.stream_of(rows)[5].tolist()
    r, seg, kv, st = run(ss, c, range(len(c)), 0, None)  # out = NULL: the sizes, res and seg_start
    assert kv is None and st == [n, kb, vb, 0] and seg.tolist() == want_seg
    check_results(r, exp, sc.FIELDS)
    dev = ss.device
    for short in range(3):  # one entry / key byte / value byte short
        caps = [n, kb, vb]
        caps[short] -= 1
        out = guarded(n, kb, vb, dev)
        r, seg, _, st = ss.scan_raw(c.q_sst, c.lower, c.upper, c.lkind, c.ukind, 0, tuple(caps), out)
        assert st == [n, kb, vb, LSMBLK_ERR_CAPACITY] and seg.tolist() == want_seg
        check_results(r, exp, sc.FIELDS)
        assert untouched(out)
    # exactly enough: the guard bytes after the arenas stay
    out = batch.KVStream(torch.full((kb + 64,), GUARD, dtype=torch.uint8, device=dev),
                         torch.zeros(n + 1, dtype=torch.int32, device=dev),
                         torch.full((vb + 64,), GUARD, dtype=torch.uint8, device=dev),
                         torch.zeros(n + 1, dtype=torch.int32, device=dev),
                         torch.zeros(n + 1, dtype=torch.int64, device=dev), 0)
    r, seg, kv, st = ss.scan_raw(c.q_sst, c.lower, c.upper, c.lkind, c.ukind, 0, (n, kb, vb), out)
    assert st == [n, kb, vb, 0]
    check_stream(kv, rows, seg)
    assert (out.keys[kb:] == GUARD).all() and (out.vals[vb:] == GUARD).all()
    with pytest.raises(LsmBlkError):
        bad = list(c.q_sst)
        bad[3] = 99
        ss.scan(bad, c.lower, c.upper, lower_kind=c.lkind, upper_kind=c.ukind)


def test_scan_retries_on_capacity_and_filters():
    c, ss = sc.case("bs4096"), opened("bs4096")  # more bytes than scan's first guess
    exp, rows = sc.expected("bs4096", True, True)
    res, got = ss.scan(c.q_sst, c.lower, c.upper, lower_kind=c.lkind, upper_kind=c.ukind, no_filter=True, mvcc=True)
    assert got == rows and (res["n"] == exp["n"]).all()
    ts = [int(t) for t in np.random.default_rng(7).choice(sc.read_ts_values(c), len(c))]
    res, got = ss.scan(c.q_sst, c.lower, c.upper, lower_kind=c.lkind, upper_kind=c.ukind, read_ts=ts, no_filter=True,
                       mvcc=True)
    assert got == [sc.lsm_iterate(r, t) for r, t in zip(rows, ts)]


def test_every_placement_of_arenas_and_query_keys():
    """Query-key arenas at every address residue mod 4, output arenas at every residue mod 16."""
    c, ss = sc.case("bs256"), opened("bs256")
    sel = list(range(0, len(c), 7))
    exp, rows = sc.expected("bs256", False, False)
    rows = [rows[i] for i in sel]
    n, kb, vb = sizes_of(rows)
    pick = lambda x: [x[i] for i in sel]
    qs, lk, lo, uk, uo, bnd = ss.upload_ranges(pick(c.q_sst), pick(c.lower), pick(c.upper), pick(c.lkind), pick(c.ukind))
    dev, nq = ss.device, len(sel)
    for r16 in range(16):
        shift = lambda t, r: torch.cat([torch.zeros(r, dtype=torch.uint8, device=dev), t])[r:]
        lk2, uk2 = shift(lk, 16 + r16 % 4), shift(uk, 16 + (r16 // 4) % 4)
        assert lk2.data_ptr() % 4 == r16 % 4 and uk2.data_ptr() % 4 == (r16 // 4) % 4
        keys = torch.full((kb + 96,), GUARD, dtype=torch.uint8, device=dev)
        vals = torch.full((vb + 96,), GUARD, dtype=torch.uint8, device=dev)
        ko, vo = 16 + r16, 16 + (r16 * 5 + 3) % 16
        out = batch.KVStream(keys[ko:ko + kb + 16], torch.zeros(n + 1, dtype=torch.int32, device=dev),
                             vals[vo:vo + vb + 16], torch.zeros(n + 1, dtype=torch.int32, device=dev),
                             torch.zeros(n + 1, dtype=torch.int64, device=dev), 0)
        assert out.keys.data_ptr() % 16 == r16 and out.vals.data_ptr() % 16 == (r16 * 5 + 3) % 16
        res = torch.zeros(nq * ctypes.sizeof(ScanResultC), dtype=torch.uint8, device=dev)
        seg = torch.zeros(nq + 1, dtype=torch.int32, device=dev)
        stats = torch.zeros(4, dtype=torch.int64, device=dev)
        ss.scan_into(qs, lk2, lo, uk2, uo, bnd, nq, 0, res, seg, stats, out, (n, kb, vb))
        torch.cuda.synchronize()
        assert stats.tolist() == [n, kb, vb, 0]
        out.n = n
        check_stream(out, rows, seg.cpu().numpy().view(np.uint32))
        check_results(res.cpu().numpy().view(np.dtype(ScanResultC)), exp, sc.FIELDS, sel)
        assert (keys[:ko] == GUARD).all() and (keys[ko + kb:] == GUARD).all()
        assert (vals[:vo] == GUARD).all() and (vals[vo + vb:] == GUARD).all()


def test_two_calls_on_one_context_are_identical():
    c, ss = sc.case("many_blocks"), opened("many_blocks")
    _, rows = sc.expected("many_blocks", False, False)
    caps = sizes_of(rows)
    a = run(ss, c, range(len(c)), 0, caps)
    b = run(ss, c, range(len(c)), 0, caps)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist() and a[3] == b[3]
    for x, y in zip(a[2].to_numpy(), b[2].to_numpy()):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("budget", (0, 5))
@pytest.mark.parametrize("nq", sc.query_counts())
def test_query_counts_and_blocks_per_unit(nq, budget):
    """1 .. kScanWg + 1 ranges per call, with the default unit budget (a block per unit) and with 5
    units for all the blocks (every unit walks several blocks)."""
    c, ss = sc.case("many_blocks"), opened("many_blocks")
    exp, rows = sc.expected("many_blocks", False, True)
    sel = list(range(nq))
    rows = [rows[i] for i in sel]
    h = batch._ctx(ss.device.index, ss.stream)
    assert lib().lsmblk_debug_set(h, LSMBLK_DEBUG_SCAN_UNITS, budget) == 0
    try:
        r, seg, kv, st = run(ss, c, sel, 2, sizes_of(rows))
    finally:
        assert lib().lsmblk_debug_set(h, LSMBLK_DEBUG_SCAN_UNITS, 0) == 0
    assert st == list(sizes_of(rows)) + [0]
    check_results(r, exp, sc.FIELDS, sel)
    check_stream(kv, rows, seg)


def test_degenerate_inputs():
    c = sc.case("bs256")
    ss = opened("bs256")
    r, seg, kv, st = ss.scan_raw([], [], [], [], [], 0, (4, 16, 16))  # nq = 0
    assert st == [0, 0, 0, 0] and len(r) == 0 and seg.tolist() == [0] and kv.n == 0
    assert ss.scan([], [], [], lower_kind=[], upper_kind=[])[1] == []
    # an SST whose open failed answers EMPTY, the others as before
    bad = 1
    bufs = [sc.corrupt_footer(s.buf) if i == bad else s.buf for i, s in enumerate(c.ssts)]
    broken = sst.SstSet(b"".join(bufs), c.file_off)
    assert broken.num_of_blocks(bad) == 0
    exp, rows = sc.expected("bs256", False, False)
    other = np.array(c.q_sst) != bad
    rows = [r_ if o else [] for r_, o in zip(rows, other)]
    r, seg, kv, st = broken.scan_raw(c.q_sst, c.lower, c.upper, c.lkind, c.ukind, 0, sizes_of(rows))
    assert st == list(sizes_of(rows)) + [0]
    check_stream(kv, rows, seg)
    check_results(r[other], exp, sc.FIELDS, other)
    assert (r["status"][~other] == sc.EMPTY).all() and (r["n"][~other] == 0).all()
    assert all((r[f][~other] == sc.NONE).all() for f in ("blk0", "ent0", "blk1", "ent1"))
    # q_sst >= nsst and an empty bounded key: flagged, those ranges empty, the others answered
    s0 = c.ssts[0]
    k0, k1 = s0.entries[5][0], s0.entries[40][0]
    want = sc.scan_one(s0, 1, k0, 1, k1, False, False)
    r, seg, kv, st = ss.scan_raw([0, 9, 0], [k0, k0, k0], [k1, k1, k1], 1, 1, 0, (1000, 8000, 30000))
    assert st[3] == LSMBLK_ERR_SEGMENTS and r["n"].tolist() == [want["n"], 0, want["n"]] and r["blk0"][1] == sc.NONE
    check_stream(kv, [want["entries"], [], want["entries"]], seg)
    r, seg, kv, st = ss.scan_raw([0, 0, 0, 0], [k0, b"", k0, b""], [k1, k1, b"", b""], [1, 2, 1, 0], [1, 1, 2, 0], 0,
                                 (4000, 30000, 90000))
    assert st[3] == LSMBLK_ERR_EMPTY_KEY and r["status"].tolist() == [sc.OK, sc.EMPTY, sc.EMPTY, sc.OK]
    assert r["n"].tolist() == [want["n"], 0, 0, len(s0.entries)]


def test_a_malformed_block_empties_its_ranges_only():
    """An entry offset pointing past the block's data: every range visiting the block is EMPTY with
    MALFORMED raised (the scan does not check CRCs), the others are answered."""
    c = sc.case("bs256")
    s = c.ssts[0]
    victim = len(s.blocks) // 2
    buf = bytearray(s.buf)
    end = s.ends[victim] - 4  # the block's end: u16 offsets, u16 count
    n = len(s.blocks[victim])
    buf[end - 2 - 2 * n:end - 2 * n] = (0xFFF0).to_bytes(2, "big")  # entry 0's offset
    ss = sst.SstSet(bytes(buf) + b"".join(x.buf for x in c.ssts[1:]), c.file_off)
    exp, rows = sc.expected("bs256", True, True)
    sel = [i for i in range(len(c)) if c.q_sst[i] == 0][:300]
    # a range visits the victim when it holds one of its entries or one of its bounds is searched there
    vk0, vk1 = s.blocks[victim][0][0], s.blocks[victim + 1][0][0]
    hits = lambda i: any(k and vk0 <= k < vk1 for k in (c.lower[i], c.upper[i])) or \
        (exp["n"][i] and exp["blk0"][i] <= victim <= exp["blk1"][i])
    clean = [i for i in sel if not hits(i) and not (exp["blk0"][i] <= victim <= exp["blk1"][i])]
    dirty = [i for i in sel if exp["n"][i] and exp["blk0"][i] < victim < exp["blk1"][i]]
    assert clean and dirty
    r, seg, kv, st = run(ss, c, clean + dirty, 3, (200000, 2000000, 6000000))
    assert st[3] == LSMBLK_ERR_MALFORMED
    check_results(r[:len(clean)], exp, sc.FIELDS, clean)
    assert (r["status"][len(clean):] == sc.EMPTY).all() and (r["n"][len(clean):] == 0).all()
    check_stream(kv, [rows[i] for i in clean] + [[] for _ in dirty], seg)


@pytest.mark.parametrize("name", ("bs128", "threshold", "ties"))
def test_included_begin_equals_the_point_reads_landing(name):
    """(blk0, ent0) of an Included lower bound == (blk, ent) of lsmblk_sst_get_batch with NO_FILTER."""
    c, ss = sc.case(name), opened(name)
    sel = [i for i in range(len(c)) if c.lkind[i] == sc.INCLUDED]
    for mvcc in (False, True):
        r, _, _, st = run(ss, c, sel, 1 | (2 if mvcc else 0), None)
        g = ss.get([c.q_sst[i] for i in sel], [c.lower[i] for i in sel], 0, no_filter=True, mvcc=mvcc, values=False)
        assert st[3] == 0
        assert (r["blk0"] == g["blk"]).all() and (r["ent0"] == g["ent"]).all()


# ------------------------------------------------------------------------------ the read filter
def kv_of(rows):
    kb, ko, vb, vo, ts, seg = sc.stream_of(rows)
    return batch.KVStream.from_numpy(np.frombuffer(kb, np.uint8), ko, np.frombuffer(vb, np.uint8), vo, ts), seg


def filtered(kv, seg, ts, caps=None, out=None):
    dev = kv.key_off.device
    nseg = len(seg) - 1
    ss = batch._u32_table(seg, dev)
    tt = torch.from_numpy(np.asarray(ts, np.uint64).view(np.int64).copy()).to(dev) if nseg else torch.zeros(1, dtype=torch.int64, device=dev)
    oss = torch.full((nseg + 1,), -1, dtype=torch.int32, device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    if out is None:
        out = batch.KVStream.empty(*caps, dev)
    batch.read_filter_into(kv, ss, tt, nseg, out, oss, stats, caps=caps)
    torch.cuda.synchronize()
    return out, oss.cpu().numpy().view(np.uint32), stats.tolist()


@pytest.mark.parametrize("name", sc.CASES)
def test_read_filter_over_scan_output(name):
    c, ss = sc.case(name), opened(name)
    _, rows = sc.expected(name, True, False)
    caps = sizes_of(rows)
    _, seg, kv, st = run(ss, c, range(len(c)), 1, caps)
    assert st[3] == 0
    tv = sc.read_ts_values(c)
    ts = [tv[i % len(tv)] for i in range(len(c))]
    want = [sc.lsm_iterate(r, t) for r, t in zip(rows, ts)]
    out, oseg, st = filtered(kv, seg, ts, sizes_of(want))
    assert st == list(sizes_of(want)) + [0]
    out.n = st[0]
    check_stream(out, want, oseg)
    got, gseg = batch.read_filter(kv, seg, ts)
    check_stream(got, want, gseg)


def test_read_filter_capacity_contract():
    c, ss = sc.case("bs256"), opened("bs256")
    _, rows = sc.expected("bs256", True, True)
    kv, seg = kv_of(rows)
    ts = [500] * len(rows)
    want = [sc.lsm_iterate(r, 500) for r in rows]
    n, kb, vb = sizes_of(want)
    dev = kv.key_off.device
    for short in range(3):
        caps = [n, kb, vb]
        caps[short] -= 1
        out = guarded(n, kb, vb, dev)
        _, oseg, st = filtered(kv, seg, ts, tuple(caps), out)
        assert st == [n, kb, vb, LSMBLK_ERR_CAPACITY]
        assert untouched(out)
    out = batch.KVStream(torch.full((kb + 64,), GUARD, dtype=torch.uint8, device=dev)[5:],
                         torch.zeros(n + 1, dtype=torch.int32, device=dev),
                         torch.full((vb + 64,), GUARD, dtype=torch.uint8, device=dev)[11:],
                         torch.zeros(n + 1, dtype=torch.int32, device=dev),
                         torch.zeros(n + 1, dtype=torch.int64, device=dev), 0)
    _, oseg, st = filtered(kv, seg, ts, (n, kb, vb), out)
    assert st == [n, kb, vb, 0]
    out.n = n
    check_stream(out, want, oseg)
    assert (out.keys[kb:] == GUARD).all() and (out.vals[vb:] == GUARD).all()
    # a decreasing segment table is refused
    bad = seg.copy()
    bad[3], bad[4] = bad[4] + 1, bad[3]
    _, _, st = filtered(kv, bad, ts, (n, kb, vb))
    assert st[3] & LSMBLK_ERR_SEGMENTS


def test_read_filter_segment_boundaries_and_long_version_runs():
    """A segment boundary between two versions of one key (nothing is compared across it), a key
    with more versions than one flag tile, empty segments, and entries outside every segment."""
    nver = sc.kFiltTile + 300
    long_key = [(b"long", nver + 10 - i, b"v%d" % i if i % 3 else b"") for i in range(nver)]
    a = [(b"a", 9, b"a9"), (b"a", 5, b"a5"), (b"b", 7, b""), (b"b", 3, b"b3")]
    rows = [a[:1], a[1:], [], long_key[:700], long_key[700:], [], a]
    outside = [(b"a", 1, b"dropped")]
    kv, seg = kv_of([outside] + rows + [outside])
    seg = seg[1:-1]  # the first and the last entry belong to no segment
    ts = [100, 100, 100, 649, 499, 5, 6]
    want = [sc.lsm_iterate(r, t) for r, t in zip(rows, ts)]
    assert want[0] == [(b"a", 9, b"a9")] and want[1] == [(b"a", 5, b"a5")]  # kept on both sides of the boundary
    assert want[6] == [(b"a", 5, b"a5"), (b"b", 3, b"b3")]
    assert len(want[3]) == 1 and len(want[4]) == 1
    out, oseg, st = filtered(kv, seg, ts, sizes_of(want))
    assert st == list(sizes_of(want)) + [0]
    out.n = st[0]
    check_stream(out, want, oseg)
    # a tombstone as the newest visible version hides the key; read_ts below every version: nothing
    for t in (0, nver // 2, nver // 2 + 1, nver + 100):
        w = [sc.lsm_iterate(long_key, t)]
        kv1, seg1 = kv_of([long_key])
        out, oseg, st = filtered(kv1, seg1, [t], (2, 16, 16))
        out.n = st[0]
        check_stream(out, w, oseg)
    out, oseg, st = filtered(*kv_of([[]]), [1], (2, 16, 16))  # an empty stream
    assert st == [0, 0, 0, 0] and oseg.tolist() == [0, 0]


# ------------------------------------------------------------------------------ composition
def test_scan_merge_read_filter_equals_lsm_iterator_over_merge_iterator():
    """Two overlapping SSTs, the newer first: scan both, lsmblk_merge_batch (LSMBLK_MERGE_RUNS) with
    the scans' seg_start as run_start, then the read filter == LsmIterator over pyref.MergeIterator
    of the same two range iterators."""
    rng = np.random.default_rng(9)
    old = gc.gen_entries(71, nkeys=500)
    keys = sorted({k for k, _, _ in old})
    new = []
    for k in keys[::2] + [k + b"x" for k in keys[::5]]:  # newer versions of half the keys, and new keys
        for ts in (2000 + int(rng.integers(0, 50)), 1500):
            new.append((k, ts, b"" if rng.random() < 0.3 else b"new-" + k))
    new.sort(key=lambda e: (e[0], -e[1]))
    ssts = [gc.make_sst(new, 256), gc.make_sst(old, 256)]
    ss = sst.SstSet(b"".join(s.buf for s in ssts), [0] + list(np.cumsum([len(s.buf) for s in ssts])))
    for lk, lo, uk, up, read_ts in ((1, keys[40], 1, keys[300], 1 << 60), (2, keys[41], 2, keys[120], 1700),
                                    (0, b"", 1, keys[200], 600), (1, keys[100][:1], 0, b"", 2020), (0, b"", 0, b"", 0)):
        for mvcc in (False, True):
            runs = [sc.scan_one(s, lk, lo, uk, up, False, mvcc)["entries"] for s in ssts]
            merged = pyref.drain(pyref.MergeIterator([pyref.ListIter(r) for r in runs]))
            # the quirk of LsmIterator::new cannot show: the first merged entry is within the upper bound
            assert merged and (uk == 0 or (merged[0][0] <= up if uk == 1 else merged[0][0] < up))
            want = sc.lsm_iterate(merged, read_ts, (uk, up))
            r, seg, kv, st = ss.scan_raw([0, 1], [lo, lo], [up, up], lk, uk, 2 if mvcc else 0, sizes_of(runs))
            assert st[3] == 0
            check_stream(kv, runs, seg)
            m = batch.merge_runs(kv, seg)
            got, gseg = batch.read_filter(m, [0, m.n], read_ts)
            check_stream(got, [want], gseg)
