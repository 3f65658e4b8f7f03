"""The snapshot-preserving merge (LSMBLK_MERGE_NEWEST) on the device, through the C ABI against the
expectations of merge_newest_cases.py (coverage asserted on the CPU by test_merge_newest_cases.py):
the merged stream entry for entry on every case, lsmblk_compact_batch byte for byte against the
oracle's compact_generate_sst over the newest order, the capacity contract, the key-range form and
the shard calls, the error contract, and the reason for the mode: a snapshot scan of an LSM view
returns the same rows before and after a NEWEST compaction, and not after a RUNS one."""
import ctypes

import numpy as np
import pytest
import torch

import lsm_get_cases as lc
import lsm_scan_cases as ls
import lsm_scan_newest_cases as ln
import merge_newest_cases as mn
from gpu_kit import GUARD, _need_gpu, guarded, untouched  # noqa: F401 (_need_gpu: autouse)
from lsm_amd import batch, shard, sst
from lsm_amd._lib import (LSMBLK_E_CAPACITY, LSMBLK_E_INVAL, LSMBLK_E_MALFORMED, LSMBLK_GET_FOUND, LSMBLK_MERGE_RUNS,
                          LSMBLK_MERGE_TWO_LEVEL, LsmBlkError)
from oracle import oracle as O
from oracle import pyref
from test_gpu_compact import assert_kv_equal, dev_entries, kv_runs, to_dev

pytestmark = pytest.mark.gpu
NEWEST, RUNS, TWO = mn.NEWEST, LSMBLK_MERGE_RUNS, LSMBLK_MERGE_TWO_LEVEL


_cases = {}


def cases():
    if not _cases:
        _cases.update(mn.merge_cases())
    return _cases


def merge_raw(d, rs, mode, out=None, caps=None):
    """lsmblk_merge_batch_ex -> (out stream, stats words); caps: the capacities declared for `out`."""
    dev = torch.device("cuda")
    rt = batch._u32_table(rs, dev)
    if out is None:
        kb, vb = d.byte_sizes()
        out = batch.KVStream.empty(d.n, kb, vb, dev)
    stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device=dev)
    ci, co = d._c(), out._c(*(caps or out.caps()))
    di = torch.cuda.current_device()
    batch._native("lsmblk_merge_batch_ex", di, None, ctypes.byref(ci), rt.data_ptr(), rt.numel() - 1, mode,
                  ctypes.byref(co), stats.data_ptr(), batch._stream_ptr(None, di))
    torch.cuda.synchronize()
    return out, stats.cpu().tolist()


# ---------------------------------------------------------------- merge parity
@pytest.mark.parametrize("name", sorted(mn.merge_cases()))
def test_merge_equals_the_newest_order_entry_for_entry(name):
    case = cases()[name]
    want = O.gather(case.kv, mn.newest_order(case))
    got, s = merge_raw(to_dev(case.kv), case.rs, NEWEST)
    assert s[3] == 0, s
    got.n = s[0]
    assert_kv_equal(got, want)
    assert s[:3] == [case.kv.n, int(want.key_off[-1]), int(want.val_off[-1])]
    assert_kv_equal(batch.merge_runs(to_dev(case.kv), case.rs, merge_mode=NEWEST), want)


# ---------------------------------------------------------------- compaction parity
def check_compact_newest(case, wm, bottom, pf, bs, target):
    src, want = mn.expected_compact(case, wm, bottom, pf, bs, target)
    got = batch.compact_runs(to_dev(case.kv), case.rs, wm, bottom, pf, bs, target, merge_mode=NEWEST)
    kept = O.gather(case.kv, src[want["kept"]])
    assert_kv_equal(got["kept"], kept)
    np.testing.assert_array_equal(got["blk_off"].cpu().numpy().view(np.uint64), want["blk_off"])
    assert got["blocks"].cpu().numpy().tobytes() == want["blocks"].tobytes()
    np.testing.assert_array_equal(got["sst_start"].cpu().numpy().view(np.uint32), want["sst_ent"])
    np.testing.assert_array_equal(got["sst_blk"].cpu().numpy().view(np.uint32), want["sst_blk"])
    assert got["stats"] == [len(want["blk_off"]) - 1, len(want["blocks"]), len(want["sst_blk"]) - 1, 0, case.kv.n,
                            kept.n, int(kept.key_off[-1]), int(kept.val_off[-1])]
    return got, want


_rules = {name: rest for name, *rest in mn.rules_cases()}


@pytest.mark.parametrize("name", sorted(_rules))
def test_compaction_equals_the_oracle_over_the_newest_order_rules(name):
    check_compact_newest(*_rules[name])


@pytest.mark.parametrize("bottom", [False, True])
def test_compaction_equals_the_oracle_over_the_newest_order_rotation(bottom):
    case = cases()["rotation"]
    got, want = check_compact_newest(case, 0, bottom, (), mn.ROT_BS, mn.ROT_TARGET)
    assert got["stats"][2] > 20
    check_compact_newest(case, 75, bottom, (b"rot-001",), mn.ROT_BS, mn.ROT_TARGET)


@pytest.mark.parametrize("name", ["cand_edges", "many_runs", "empty_runs", "tile_%d" % mn.C.kMTE,
                                  "tile_%d" % (mn.C.kBigTE + 1)])
def test_compaction_equals_the_oracle_over_the_newest_order_paths(name):
    case = cases()[name]
    tss = sorted(case.kv.ts.tolist())
    wm = tss[len(tss) // 2] if tss else 0
    check_compact_newest(case, wm, True, (), 256, 2000)


# ---------------------------------------------------------------- capacity contract
def test_an_out_stream_one_short_reports_capacity_and_writes_nothing():
    case = cases()["key_ties"]
    d, n = to_dev(case.kv), case.kv.n
    kb, vb = int(case.kv.key_off[-1]), int(case.kv.val_off[-1])
    for short in range(3):
        caps = [n, kb, vb]
        caps[short] -= 1
        out = guarded(n, kb, vb)
        _, s = merge_raw(d, case.rs, NEWEST, out, tuple(caps))
        assert s == [n, kb, vb, s[3]] and batch._status(torch.tensor(s)) == LSMBLK_E_CAPACITY, (short, s)
        assert untouched(out), short
    out = guarded(n, kb, vb)   # exactly enough
    _, s = merge_raw(d, case.rs, NEWEST, out, (n, kb, vb))
    assert s == [n, kb, vb, 0]
    out.n = n
    assert_kv_equal(out, O.gather(case.kv, mn.newest_order(case)))
    assert bool((out.keys[kb:] == GUARD).all() and (out.vals[vb:] == GUARD).all())


# ---------------------------------------------------------------- key-range form and the shard calls
@pytest.mark.parametrize("name,wm,bottom", [("interleaved", 6, True), ("many_runs", 4, False), ("rotation", 75, True),
                                            ("cand_edges", 3800, False)])
def test_key_ranges_concatenate_to_the_unsplit_kept_stream_and_blocks(name, wm, bottom):
    case = cases()[name]
    bs, target = mn.ROT_BS, mn.ROT_TARGET
    src, want = mn.expected_compact(case, wm, bottom, (), bs, target)
    kept = [case.kv.entry(int(i)) for i in src[want["kept"]]]
    d = to_dev(case.kv)
    opts = batch.compact_opts(wm, bottom, block_size=bs, target_sst_size=target, merge_mode=NEWEST)
    multi = sorted(k for k in mn.multi_run_keys(case) if sum(k in {e[0] for e in r} for r in case.runs()) >= 3)
    keys = sorted({e[0] for e in case.kv.entries()})
    assert multi and len(keys) >= 6
    picks = sorted({multi[0]} | {keys[i * len(keys) // 5] for i in range(1, 5)})
    while len(picks) > 4:
        picks.remove(next(k for k in picks if k != multi[0]))
    assert len(picks) == 4
    single = batch.compact_runs(d, case.rs, wm, bottom, (), bs, target, merge_mode=NEWEST)
    for sp in ([], [multi[0]], picks):   # 1, 2 and 5 ranges; a splitter equal to a key that lives in three runs
        parts = []
        shards = [shard.RangeShard(d, case.rs, opts, *shard.range_of(r, sp)) for r in range(len(sp) + 1)]
        res = shard.compact_local(shards)   # compact_merge_into, then halo, shard_prepare / carry / encode_into
        for r, sh in enumerate(shards):
            lo, hi = shard.range_of(r, sp)
            k, s = sh.kept, sh.mstats.cpu().tolist()
            got = dev_entries(batch.KVStream(k.keys, k.key_off, k.vals, k.val_off, k.ts, sh.m))
            assert s[3] == 0 and s[4] == case.kv.n and s[0] == len(got) == res[r]["m"]
            assert all((lo is None or e[0] >= lo) and (hi is None or e[0] < hi) for e in got)
            parts += got
        assert parts == kept, len(sp)
        assert b"".join(r["blocks"].cpu().numpy().tobytes() for r in res) == single["blocks"].cpu().numpy().tobytes() \
            == want["blocks"].tobytes()
        bases = np.concatenate([[0], np.cumsum([r["m"] for r in res])]).tolist()
        assert bases[-1] == len(kept) and shard.sst_starts(res, bases) == want["sst_ent"][:-1].tolist()
        for a, b in zip(res, res[1:]):
            assert a["carry_out"] == b["carry_in"]


# ---------------------------------------------------------------- error contract
def status_of(fn):
    with pytest.raises(LsmBlkError) as e:
        fn()
    return e.value.status


def test_a_run_out_of_order_is_malformed_wherever_it_lands():
    it = cases()["interleaved"]
    runs = it.runs()
    swapped = [list(r) for r in runs]
    swapped[1][1], swapped[1][2] = swapped[1][2], swapped[1][1]   # b-only@2 after k-inter@7: a key decreases
    assert swapped[1][1][0] > swapped[1][2][0]
    rising = [list(r) for r in runs]
    rising[2][0], rising[2][1] = rising[2][1], rising[2][0]       # k-inter 5 before 8 in run 2: the keys stay sorted
    assert rising[2][0][0] == rising[2][1][0] and rising[2][0][1] < rising[2][1][1]
    big = cases()["tile_%d" % (mn.C.kBigTE + 1)].runs()            # the same deep inside a tile of the global path
    j = len(big[1]) // 2
    assert big[1][j][0] == big[1][j + 1][0]
    big[1][j], big[1][j + 1] = big[1][j + 1], big[1][j]
    for bad in (swapped, rising, big):
        kv, rs = kv_runs(bad)
        d = to_dev(kv)
        assert status_of(lambda: batch.merge_runs(d, rs, merge_mode=NEWEST)) == LSMBLK_E_MALFORMED
        assert status_of(lambda: batch.compact_runs(d, rs, 5, False, (), 256, 1000, merge_mode=NEWEST)) == LSMBLK_E_MALFORMED
    kv, rs = kv_runs(rising)   # the run-priority merge never looks at the ts
    assert batch.merge_runs(to_dev(kv), rs, merge_mode=RUNS).n > 0


def test_other_modes_counts_and_key_lengths_are_refused():
    case = cases()["interleaved"]
    d = to_dev(case.kv)
    for mode in (3, 4, 0xFFFFFFFF):
        assert status_of(lambda: batch.merge_runs(d, case.rs, merge_mode=mode)) == LSMBLK_E_INVAL
        assert status_of(lambda: batch.compact_runs(d, case.rs, 0, False, (), 4096, 1 << 20, merge_mode=mode)) == LSMBLK_E_INVAL
        opts = batch.compact_opts(0, False, block_size=4096, target_sst_size=1 << 20, merge_mode=mode)
        assert status_of(lambda: shard.RangeShard(d, case.rs, opts).merge()) == LSMBLK_E_INVAL
    kv, rs = kv_runs([[(b"k%02d" % r, 1, b"v")] for r in range(65)])   # nrun == 65
    for mode in (RUNS, NEWEST):
        assert status_of(lambda: batch.merge_runs(to_dev(kv), rs, merge_mode=mode)) == LSMBLK_E_INVAL
    kv, rs = kv_runs([[(b"k" * 65536, 2, b"x")], [(b"k", 1, b"y")]])   # a 65 536-byte key
    for mode in (RUNS, NEWEST):
        assert status_of(lambda: batch.merge_runs(to_dev(kv), rs, merge_mode=mode)) == LSMBLK_E_INVAL
        assert status_of(lambda: batch.compact_runs(to_dev(kv), rs, 0, False, (), 4096, 1 << 20, merge_mode=mode)) == LSMBLK_E_INVAL
    kv, rs = kv_runs([[(b"k" * 65535, 2, b"x")], [(b"k", 1, b"y"), (b"k" * 65535, 3, b"z")]])   # 65 535 bytes still merge
    assert [e[1:] for e in dev_entries(batch.merge_runs(to_dev(kv), rs, merge_mode=NEWEST))] == [(1, b"y"), (3, b"z"), (2, b"x")]


@pytest.mark.parametrize("name", ["interleaved", "key_ties"])
def test_modes_0_and_1_still_equal_their_references(name):
    case = cases()[name]
    d, runs = to_dev(case.kv), case.runs()
    src = O.merge_runs(case.kv, case.rs)
    assert_kv_equal(batch.merge_runs(d, case.rs, merge_mode=RUNS), O.gather(case.kv, src))
    assert dev_entries(batch.merge_runs(d, case.rs, merge_mode=TWO)) == pyref.two_merge_rule(runs)
    want = O.compact(case.kv, src, 5, True, (), 64, 100)
    got = batch.compact_runs(d, case.rs, 5, True, (), 64, 100, merge_mode=RUNS)
    assert got["blocks"].cpu().numpy().tobytes() == want["blocks"].tobytes()
    np.testing.assert_array_equal(got["sst_start"].cpu().numpy().view(np.uint32), want["sst_ent"])
    assert_kv_equal(got["kept"], O.gather(case.kv, src[want["kept"]]))


# ---------------------------------------------------------------- end to end: snapshot reads before and after
BS = 128


def open_versions():
    """The `versions` view of lsm_scan_newest_cases.py (L0 a, L0 b, level 0 = {c1}, level 1 = {c2})
    encoded on the device as SST files and opened; -> (view case, SstSet, LsmView, the tables' blocks
    decoded into one stream of runs in source order, run_start)."""
    v = ln.case("versions", BS).view
    order = ls.tables(v)
    assert order == [0, 1, 2, 3] and v.l0 == [0, 1] and v.levels == [[2], [3]]
    tabs = [lc.flat(v.ssts[t])[0] for t in order]
    kv, seg = kv_runs(tabs)
    d = to_dev(kv)
    r = batch.encode_sst(d, seg, BS)
    files, off = sst.sst_files(r["blocks"], r["blk_off"], r["seg_blk"], seg, d)
    ss = sst.SstSet(files, off)
    assert ss.open_stats[0] == 4 and ss.open_stats[3] == 0
    runs = batch.decode_blocks(r["blocks"], r["blk_off"])
    assert_kv_equal(runs, kv)
    return v, ss, ss.view(v.l0, v.levels), runs, seg, kv


def snapshot(ss, view, ranges, keys, T):
    lo, up, lk, uk = zip(*ranges)
    _, rows = ss.lsm_scan(view, list(lo), list(up), lower_kind=list(lk), upper_kind=list(uk), read_ts=T, newest=True)
    g = ss.lsm_get(view, keys, T, newest=True)
    gets = [(k, int(g["ts"][i]), g["values"][i]) if g["status"][i] == LSMBLK_GET_FOUND else None for i, k in enumerate(keys)]
    return rows, gets


@pytest.mark.parametrize("bottom", [False, True])
@pytest.mark.parametrize("wm", [300, 500])
def test_snapshot_reads_are_the_same_after_a_newest_compaction_and_not_after_a_runs_one(wm, bottom):
    v, ss, view, runs, seg, kv = open_versions()
    k = lambda x: ln.T + x
    ranges = [(b"", b"", ln.UNBOUNDED, ln.UNBOUNDED), (k(b"e"), k(b"n"), ln.INCLUDED, ln.EXCLUDED),
              (k(b"m-many"), k(b"x-inter"), ln.EXCLUDED, ln.INCLUDED), (k(b"r0003"), k(b"r0090"), ln.INCLUDED, ln.INCLUDED)]
    keys = sorted({e[0] for e in kv.entries()})
    reads = (wm, wm + 1, 750, mn.U64)   # 750: between b's 700 and c2's 800 of x-inter
    assert all(T >= wm for T in reads)
    before = {T: snapshot(ss, view, ranges, keys, T) for T in reads}
    ents = kv.entries()
    for T in reads:   # the device's rows are the plain per-key maximum over every input entry
        assert before[T][0][0] == mn.snapshot_rows([ents[int(i)] for i in mn.newest_order(mn.cc.Case(kv, seg))], T)
        assert sum(g is not None for g in before[T][1]) == len(before[T][0][0])
    after = {}
    for mode in (NEWEST, RUNS):
        r = batch.compact_runs(runs, seg, wm, bottom, (), BS, 1000, merge_mode=mode)
        assert r["stats"][2] >= 2 and r["stats"][3] == 0   # a level of several tables
        ss2, view2 = sst.open_compacted(r)
        assert ss2.nsst == r["stats"][2] and not ss2.err.any()
        after[mode] = {T: snapshot(ss2, view2, ranges, keys, T) for T in reads}
    for T in reads:
        assert after[NEWEST][T][0] == before[T][0], T   # every range's rows (key, ts, value)
        assert after[NEWEST][T][1] == before[T][1], T   # every key's point read
    differing = [(T, q) for T in reads for q in range(len(ranges)) if after[RUNS][T][0][q] != before[T][0][q]]
    assert differing and any(a != b for T in reads for a, b in zip(after[RUNS][T][1], before[T][1]))
    rows750 = {e[0]: e for e in before[750][0][0]}
    assert rows750[k(b"x-inter")][1:] == (700, b"b700")   # the version a RUNS compaction loses: only a's 900, 300 remain
    assert {e[0]: e for e in after[RUNS][750][0][0]}[k(b"x-inter")][1:] == (300, b"a300")
