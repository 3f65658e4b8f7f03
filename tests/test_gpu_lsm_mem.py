"""Memtable runs as sources of the LSM point reads and range scans on the device (lsmblk_lsm_view.mem;
lsm_amd.sst.mem_runs / LsmView(mem=...)) against the closed forms of lsm_mem_cases.py: every field of
every result in the three point-read modes with the values gathered from both arenas, every result
field, seg_start, the eight stats words and every byte of raw and out in the five scan modes, the
capacity contracts, the equivalence with the same runs flushed to L0 tables, the error contract, a
database without an SST, and a MemTable read before and after its flush."""
import ctypes

import numpy as np
import pytest
import torch

import lsm_mem_cases as mc
import scan_cases as sc
from gpu_kit import (GUARD, _need_gpu, all_empty, check_results, check_stream,  # noqa: F401 (_need_gpu: autouse)
                     guarded, opened_view, sizes_of, untouched)
from lsm_amd import batch, sst
from lsm_amd._lib import (LSMBLK_ERR_CAPACITY, LSMBLK_ERR_SEGMENTS, LSMBLK_E_INVAL, KVStreamC, LsmBlkError,
                          LsmGetResultC, LsmScanResultC, LsmViewC)

pytestmark = pytest.mark.gpu


def device_runs(c):
    """The case's runs on the device as LsmView takes them: (the runs' KVStream, run_start)."""
    kb, ko, vb, vo, ts, start = c.stream()
    kv = batch.KVStream.from_numpy(np.frombuffer(kb, np.uint8), ko, np.frombuffer(vb, np.uint8), vo, ts)
    return kv, batch._u32_table(start, kv.keys.device)


def opened(name, bs):
    """(the case, the SstSet of its tables, its view with the runs); tables of the same view are opened once."""
    c = mc.case(name, bs)
    return (c, *opened_view(c.view, ("lsm_mem", name, bs), mem=lambda: device_runs(c),
                            set_key=("lsm_mem", c.view.name, bs)))


def check_fields(got, exp, keys, what=""):
    for f in mc.GET_FIELDS:
        bad = np.nonzero(got[f].astype(np.uint64) != exp[f])[0]
        assert not len(bad), (what, f, bad[:5], [keys[i] for i in bad[:5]], got[f][bad[:5]], exp[f][bad[:5]])


# ------------------------------------------------------------------------------ point reads
@pytest.mark.parametrize("mode", mc.GET_MODES)
@pytest.mark.parametrize("name,bs", mc.CASES)
def test_get_every_field_and_value_equals_the_closed_form(name, bs, mode):
    c, ss, view = opened(name, bs)
    exp, values, val_off = mc.get_expected(name, bs, mode)
    need, nq = int(val_off[-1]), len(c.keys)
    buf = torch.full((need + 65,), GUARD, dtype=torch.uint8, device="cuda")
    vals = buf[1:]  # an unaligned value arena
    r, _, vo, st = ss.lsm_get_raw(view, c.keys, c.read_ts, mc.GET_FLAGS[mode], val_cap=need, vals=vals)  # exact capacity
    check_fields(r, exp, c.keys)
    assert st == [nq, int((exp["status"] == mc.FOUND).sum()), need, 0]
    assert vo.tolist() == val_off.tolist()
    assert vals[:need].cpu().numpy().tobytes() == b"".join(x for x in values if x)
    assert (vals[need:] == GUARD).all() and buf[0].item() == GUARD
    # val_pos / vlen point at the value in the arena the source names
    files, memv = c.view.files, c.stream()[2]
    for i in np.nonzero(r["status"] == mc.FOUND)[0][:300]:
        arena = memv if r["src"][i] < c.nmem else files
        assert arena[int(r["val_pos"][i]):int(r["val_pos"][i]) + int(r["vlen"][i])] == values[i]
    out = ss.lsm_get(view, c.keys, c.read_ts, mvcc=mode == "mvcc", newest=mode == "newest")
    assert out["values"] == values and all((out[f] == r[f]).all() for f in mc.GET_FIELDS)


@pytest.mark.parametrize("mode", mc.GET_MODES)
def test_get_capacity_carries_the_bytes_and_writes_nothing(mode):
    c, ss, view = opened("mixed3", 128)
    exp, values, val_off = mc.get_expected("mixed3", 128, mode)
    need, nq = int(val_off[-1]), len(c.keys)
    mem_bytes = sum(len(v) for v, s in zip(values, exp["src"]) if v and s < c.nmem)
    assert 0 < mem_bytes < need  # values of both arenas
    vals = torch.full((need + 64,), GUARD, dtype=torch.uint8, device="cuda")
    r, _, vo, st = ss.lsm_get_raw(view, c.keys, c.read_ts, mc.GET_FLAGS[mode], val_cap=need - 1, vals=vals)  # one byte short
    assert st == [nq, int((exp["status"] == mc.FOUND).sum()), need, LSMBLK_ERR_CAPACITY] and (vals == GUARD).all()
    check_fields(r, exp, c.keys, "short")
    r2, none, vo2, st2 = ss.lsm_get_raw(view, c.keys, c.read_ts, mc.GET_FLAGS[mode])  # vals = NULL
    assert none is None and vo2 is None and st2 == [nq, st[1], 0, 0]
    check_fields(r2, exp, c.keys, "no gather")


# ------------------------------------------------------------------------------ range scans
def scan(ss, view, c, sel, mode, raw_caps, out_caps, **kw):
    s = c.scan
    pick = lambda x: [x[i] for i in sel]
    flags, filt = mc.scan_mode_args(mode)
    return ss.lsm_scan_raw(view, pick(s.lower), pick(s.upper), pick(s.lkind), pick(s.ukind), pick(s.read_ts) if filt else None,
                           flags, raw_caps=raw_caps, out_caps=out_caps, **kw)


@pytest.mark.parametrize("mode", mc.SCAN_MODES)
@pytest.mark.parametrize("name,bs", mc.CASES)
def test_scan_every_field_and_byte_equals_the_closed_form(name, bs, mode):
    c, ss, view = opened(name, bs)
    exp, out_rows, raw_runs = mc.scan_expected(name, bs, mode)
    (n, kb, vb), (rn, rkb, rvb) = sizes_of(out_rows), sizes_of(raw_runs)
    raw, out = guarded(rn, rkb, rvb, ss.device, 3), guarded(n, kb, vb, ss.device, 5)  # exact capacities, unaligned arenas
    r, seg, raw, out, st = scan(ss, view, c, range(len(c.scan)), mode, (rn, rkb, rvb), (n, kb, vb), raw=raw, out=out)
    assert st == [n, kb, vb, 0, rn, rkb, rvb, len(raw_runs)]
    check_results(r, exp, mc.SCAN_FIELDS)
    check_stream(out, out_rows, seg)
    check_stream(raw, raw_runs)
    assert (out.keys[kb:] == GUARD).all() and (out.vals[vb:] == GUARD).all()
    assert (raw.keys[rkb:] == GUARD).all() and (raw.vals[rvb:] == GUARD).all()
    if mode.endswith("merged"):
        assert (r["n"] == r["merged"]).all()
    if name in ("mixed3", "nosst"):  # the wrapper: its own sizes (view_sub_cap counts the runs), one retry at the most
        flags, filt = mc.scan_mode_args(mode)
        s = c.scan
        res, got = ss.lsm_scan(view, s.lower, s.upper, lower_kind=s.lkind, upper_kind=s.ukind,
                               read_ts=s.read_ts if filt else None, mvcc=flags == 2, newest=flags == 4)
        assert got == out_rows and all((res[f].astype(np.uint64) == exp[f]).all() for f in mc.SCAN_FIELDS)


def test_scan_three_stage_capacity_contract():
    c, ss, view = opened("mixed3", 128)
    exp, out_rows, raw_runs = mc.scan_expected("mixed3", 128, "mvcc")
    (n, kb, vb), (rn, rkb, rvb), subs, nq = sizes_of(out_rows), sizes_of(raw_runs), len(raw_runs), len(c.scan)
    want_seg = sc.stream_of(out_rows)[5].tolist()
    full = [n, kb, vb, 0, rn, rkb, rvb, subs]
    dev, sel = ss.device, range(nq)
    assert min(n, kb, vb, subs) > 1 and sst.view_sub_cap(view, nq) == nq * (3 + len(c.view.ssts))
    # no stream at all: the table scans' sizes, the runs' slices among them
    r, seg, _, _, st = scan(ss, view, c, sel, "mvcc", None, None)
    assert st == [0, 0, 0, 0, rn, rkb, rvb, subs] and seg.tolist() == [0] * (nq + 1)
    check_results(r, exp, ("sources", "raw"))
    # sub_cap one short of stats[7]: no scan runs
    raw, out = guarded(rn, rkb, rvb, dev), guarded(n, kb, vb, dev)
    r, seg, _, _, st = scan(ss, view, c, sel, "mvcc", (rn, rkb, rvb), (n, kb, vb), sub_cap=subs - 1, raw=raw, out=out)
    assert st[3] == LSMBLK_ERR_CAPACITY and st[7] == subs
    all_empty(r, seg, nq)
    assert untouched(raw, offsets=False) and untouched(out, offsets=False)
    # a capacity of raw one short
    for short in range(3):
        caps = [rn, rkb, rvb]
        caps[short] -= 1
        raw, out = guarded(rn, rkb, rvb, dev), guarded(n, kb, vb, dev)
        r, seg, _, _, st = scan(ss, view, c, sel, "mvcc", tuple(caps), (n, kb, vb), raw=raw, out=out)
        assert st == [0, 0, 0, LSMBLK_ERR_CAPACITY, rn, rkb, rvb, subs] and seg.tolist() == [0] * (nq + 1), short
        check_results(r, exp, ("sources", "raw"))
        assert (r["merged"] == 0).all() and (r["n"] == 0).all() and (r["status"] == mc.EMPTY).all()
        assert untouched(raw), short
    # a capacity of out one short
    for short in range(3):
        caps = [n, kb, vb]
        caps[short] -= 1
        raw, out = guarded(rn, rkb, rvb, dev), guarded(n, kb, vb, dev)
        r, seg, raw, _, st = scan(ss, view, c, sel, "mvcc", (rn, rkb, rvb), tuple(caps), raw=raw, out=out)
        assert st == [n, kb, vb, LSMBLK_ERR_CAPACITY, rn, rkb, rvb, subs] and seg.tolist() == want_seg, short
        check_results(r, exp, mc.SCAN_FIELDS)
        assert untouched(out), short
        raw.n = rn
        check_stream(raw, raw_runs)
    # exactly enough
    r, seg, raw, out, st = scan(ss, view, c, sel, "mvcc", (rn, rkb, rvb), (n, kb, vb), sub_cap=subs)
    assert st == full
    check_stream(out, out_rows, seg)


# ------------------------------------------------------------------------------ the runs, flushed
_flushed = {}


def flushed(name, bs):
    """The case with every run encoded as an SST and put first in l0 of a view without runs:
    (SstSet, view)."""
    if (name, bs) not in _flushed:
        c = mc.case(name, bs)
        assert all(c.runs)
        bufs = []
        for run in c.runs:
            kb, ko, vb, vo, ts, _ = sc.stream_of([run])
            d = batch.KVStream.from_numpy(np.frombuffer(kb, np.uint8), ko, np.frombuffer(vb, np.uint8), vo, ts)
            seg = np.array([0, d.n], np.uint32)
            e = batch.encode_sst(d, seg, 256)
            files, _ = sst.sst_files(e["blocks"], e["blk_off"], e["seg_blk"], seg, d)
            bufs.append(files.cpu().numpy().tobytes())
        bufs += [s.buf for s in c.view.ssts]
        ss = sst.SstSet(b"".join(bufs), [0] + [int(x) for x in np.cumsum([len(b) for b in bufs])])
        assert ss.open_stats[0] == len(bufs) and ss.open_stats[3] == 0
        m = c.nmem
        view = ss.view(list(range(m)) + [t + m for t in c.view.l0], [[t + m for t in lv] for lv in c.view.levels])
        _flushed[name, bs] = (ss, view)
    return _flushed[name, bs]


@pytest.mark.parametrize("name,bs", (("mixed3", 128), ("nosst", 0)))
def test_flush_equivalence(name, bs):
    """The same entries as memtable runs and as L0 tables in the runs' place: byte-identical scans in the
    MVCC and NEWEST modes, equal point reads (seeks / bloom_out apart: a bloom filter may reject an
    absent key that a memtable run always searches)."""
    c, ss, view = opened(name, bs)
    fs, fview = flushed(name, bs)
    s = c.scan
    for mvcc, newest in ((True, False), (False, True)):
        _, out_rows, raw_runs = mc.scan_expected(name, bs, "newest" if newest else "mvcc")
        caps = dict(raw_caps=sizes_of(raw_runs), out_caps=sizes_of(out_rows))  # (the tables' runs have the slices' sizes)
        a = ss.lsm_scan_raw(view, s.lower, s.upper, s.lkind, s.ukind, s.read_ts, 4 if newest else 2, **caps)
        b = fs.lsm_scan_raw(fview, s.lower, s.upper, s.lkind, s.ukind, s.read_ts, 4 if newest else 2, **caps)
        assert a[4][3] == 0 and b[4][3] == 0 and a[4][:3] == b[4][:3] and a[4][0] > 0
        assert a[1].tolist() == b[1].tolist()
        for x, y in zip(a[3].to_numpy(), b[3].to_numpy()):
            assert x.tobytes() == y.tobytes()
        g = ss.lsm_get(view, c.keys, c.read_ts, mvcc=mvcc, newest=newest)
        h = fs.lsm_get(fview, c.keys, c.read_ts, mvcc=mvcc, newest=newest)
        for f in ("status", "src", "ts", "vlen"):
            assert (g[f] == h[f]).all(), f
        assert g["values"] == h["values"] and any(g["values"])


# ------------------------------------------------------------------------------ the error contract
def call_get(ss, cv, nq=1):
    qk = batch._aligned_empty(16, ss.device)
    qo = batch._u32_table(np.arange(nq + 1, dtype=np.uint32), ss.device)
    qt = torch.zeros(nq, dtype=torch.int64, device=ss.device)
    res = torch.zeros(nq * ctypes.sizeof(LsmGetResultC), dtype=torch.uint8, device=ss.device)
    stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device=ss.device)
    batch._native("lsmblk_lsm_get_batch", ss.device.index, None, batch._ptr(ss.files), ss.file_off.data_ptr(), ss.nsst,
                  ss.desc_t.data_ptr(), batch._ptr(ss.index_t), ctypes.byref(cv), qk.data_ptr(), qo.data_ptr(), qt.data_ptr(),
                  nq, 0, res.data_ptr(), None, 0, None, stats.data_ptr(), batch._stream_ptr(None, ss.device.index))


def call_scan(ss, cv, nq=1):
    z = batch._u32_table(np.zeros(nq + 1, np.uint32), ss.device)
    qk = batch._aligned_empty(16, ss.device)
    res = torch.zeros(nq * ctypes.sizeof(LsmScanResultC), dtype=torch.uint8, device=ss.device)
    stats = torch.zeros(8, dtype=torch.int64, device=ss.device)
    batch._native("lsmblk_lsm_scan_batch", ss.device.index, None, batch._ptr(ss.files), ss.file_off.data_ptr(), ss.nsst,
                  ss.desc_t.data_ptr(), batch._ptr(ss.index_t), ctypes.byref(cv), qk.data_ptr(), z.data_ptr(), qk.data_ptr(),
                  z.data_ptr(), z.data_ptr(), None, nq, 0, 16, res.data_ptr(), None, None, z.data_ptr(), stats.data_ptr(),
                  batch._stream_ptr(None, ss.device.index))


def test_host_rules_give_e_inval():
    c, ss, view = opened("mixed3", 128)
    good = view._c()
    call_get(ss, good)
    call_scan(ss, good)

    def broken(change):
        cv, m = view._c(), KVStreamC.from_buffer_copy(view._mem_c)
        change(cv, m)
        if cv.mem:
            cv.mem = ctypes.pointer(m)
        return cv

    cases = [lambda cv, m: setattr(cv, "nmem", 65), lambda cv, m: setattr(cv, "mem", None),
             lambda cv, m: setattr(cv, "mem_start", None)]
    cases += [lambda cv, m, f=f: setattr(m, f, None) for f in ("keys", "key_off", "vals", "val_off", "ts")]
    for change in cases:
        for call in (call_get, call_scan):
            with pytest.raises(LsmBlkError) as e:
                call(ss, broken(change))
            assert e.value.status == LSMBLK_E_INVAL
    with pytest.raises(LsmBlkError) as e:  # the wrapper refuses a 65th run before any call
        ss.view([], [], mem=[batch.KVStream.empty(0, 0, 0, ss.device)] * 65)
    assert e.value.status == LSMBLK_E_INVAL


@pytest.mark.parametrize("start", ([1, 200, 264, 327], [0, 264, 200, 327], [0, 200, 264, 326], [0, 200, 264, 328]))
def test_a_bad_mem_start_is_refused_by_the_view_check(start):
    """A non-zero first word, a decreasing table, a last word that is not mem->n: SEGMENTS, reported as a
    bad level_start is -- no lookup and no scan runs."""
    c, ss, _ = opened("mixed3", 128)
    assert c.start == [0, 200, 264, 327]
    kv, _ = device_runs(c)
    view = ss.view(c.view.l0, c.view.levels, mem=(kv, batch._u32_table(np.array(start, np.uint32), ss.device)))
    nq = 40
    r, _, vo, st = ss.lsm_get_raw(view, c.keys[:nq], c.read_ts[:nq], 2, val_cap=4096)
    assert st == [nq, 0, 0, LSMBLK_ERR_SEGMENTS]
    assert (r["status"] == mc.ABSENT).all() and (r["vlen"] == 0).all() and (r["seeks"] == 0).all() and (r["bloom_out"] == 0).all()
    for f in ("src", "sst", "hit_blk", "hit_ent"):
        assert (r[f] == mc.NONE).all(), f
    assert vo.tolist() == [0] * (nq + 1)
    for mode in mc.SCAN_MODES:
        r, seg, raw, out, st = scan(ss, view, c, range(nq), mode, (4096, 65536, 65536), (4096, 65536, 65536))
        assert st == [0, 0, 0, LSMBLK_ERR_SEGMENTS, 0, 0, 0, 0], mode
        all_empty(r, seg, nq)
    with pytest.raises(LsmBlkError):
        ss.lsm_get(view, c.keys[:nq], c.read_ts[:nq])


# ------------------------------------------------------------------------------ no SST, and a MemTable end to end
def test_a_database_without_ssts():
    """SstSet with zero files: NULL index, nsst == 0; the view names no table and its runs answer."""
    c, ss, view = opened("nosst", 0)
    assert ss.nsst == 0 and ss.index_t is None and view.nmem == 2 and view.l0 == [] and view.levels == []
    exp, values, _ = mc.get_expected("nosst", 0, "default")
    out = ss.lsm_get(view, c.keys, c.read_ts)
    assert out["values"] == values and (out["sst"] == mc.NONE).all() and sum(v is not None for v in values) > 100
    assert all((out[f].astype(np.uint64) == exp[f]).all() for f in mc.GET_FIELDS)
    with pytest.raises(LsmBlkError) as e:  # without runs such a call names tables it cannot have
        ss.lsm_get(ss.view([0], []), c.keys[:4], c.read_ts[:4])
    assert e.value.status != 0


def rows_of(ss, view, lower, upper, kinds, read_ts, **kw):
    return ss.lsm_scan(view, lower, upper, lower_kind=kinds[0], upper_kind=kinds[1], read_ts=read_ts, **kw)[1]


def test_a_memtable_read_through_mem_runs_and_after_its_flush():
    rng = np.random.default_rng(5)
    mt = sst.MemTable()
    want = {}
    for i in range(300):
        k = b"key%04d" % int(rng.integers(0, 180))
        v = b"" if rng.random() < 0.2 else bytes(rng.integers(0, 256, int(rng.integers(1, 50)), dtype=np.uint8))
        mt.put(k, 10 + i, v)
        want[k] = (10 + i, v)  # a put of a present key replaces the entry
    assert len(mt) == len(want)
    none = sst.SstSet(b"", [0])
    kv, start = sst.mem_runs([mt], none.device)
    assert kv.n == len(want) and start.tolist() == [0, len(want)]
    view = none.view([], [], mem=(kv, start))
    keys = sorted(want) + [b"key", b"key9999", b"kez"]
    got = none.lsm_get(view, keys, 1 << 40, mvcc=True)
    assert got["values"] == [want[k][1] or None if k in want else None for k in keys]
    assert [int(t) for t in got["ts"][:len(want)]] == [want[k][0] for k in sorted(want)]
    early = none.lsm_get(view, keys, 9, mvcc=True)  # before every put: the run decides ABSENT
    assert early["values"] == [None] * len(keys) and (early["src"][:len(want)] == 0).all()
    bounds = ([b"key0010", None], [b"key0100", None], (["included", "unbounded"], ["excluded", "unbounded"]))
    rows = rows_of(none, view, *bounds, 1 << 40, mvcc=True)
    assert rows[0] == [(k, want[k][0], want[k][1]) for k in sorted(want) if b"key0010" <= k < b"key0100" and want[k][1]]
    assert rows[1] == [(k, want[k][0], want[k][1]) for k in sorted(want) if want[k][1]]
    # the same memtable, flushed: the L0 table gives the same rows
    buf = sst.flush_memtable(mt, 256)
    ss = sst.SstSet(buf, [0, len(buf)])
    l0 = ss.view([0], [])
    flushed_get = ss.lsm_get(l0, keys, 1 << 40, mvcc=True)
    assert flushed_get["values"] == got["values"] and (flushed_get["ts"] == got["ts"]).all()
    assert (flushed_get["status"] == got["status"]).all()
    assert rows_of(ss, l0, *bounds, 1 << 40, mvcc=True) == rows
    # ... and under a second, newer memtable both are sources of one view
    mt2 = sst.MemTable()
    mt2.put(b"key0010", 1000, b"newer")
    mt2.put(sorted(want)[-1], 1001, b"")
    both = ss.view([0], [], mem=[mt2])
    other = next(k for k in sorted(want) if k not in (b"key0010", sorted(want)[-1]))
    top = ss.lsm_get(both, [b"key0010", sorted(want)[-1], other], 1 << 40)
    assert top["values"][:2] == [b"newer", None] and top["src"].tolist()[:2] == [0, 0] and top["src"][2] == 1
    assert top["values"][2] == (want[other][1] or None)


def test_mem_runs_concatenates_streams_and_memtables():
    c, ss, view = opened("mixed3", 128)
    parts = []
    for run in c.runs[:2]:
        kb, ko, vb, vo, ts, _ = sc.stream_of([run])
        parts.append(batch.KVStream.from_numpy(np.frombuffer(kb, np.uint8), ko, np.frombuffer(vb, np.uint8), vo, ts))
    mt = sst.MemTable()
    last = {}
    for k, ts, v in reversed(c.runs[2]):  # the oldest version first: the newest stays
        mt.put(k, ts, v)
        last[k] = (k, ts, v)
    kv, start = sst.mem_runs(parts + [mt], ss.device)
    assert start.tolist() == [0, 200, 264, 264 + len(last)]
    want = sc.stream_of(c.runs[:2] + [[last[k] for k in sorted(last)]])
    got = kv.to_numpy()
    assert got[0].tobytes() == want[0] and got[1].tolist() == want[1].tolist() and got[2].tobytes() == want[2]
    assert got[3].tolist() == want[3].tolist() and got[4].tolist() == want[4].tolist()
    assert ctypes.sizeof(LsmViewC) == 56 and view._c().nmem == 3
