"""The key-range shard calls on every carry, bound and error: the inputs of tests/shard_cases.py (their
coverage asserted on the CPU by test_shard_cases.py) through batch.shard_prepare / shard_carry /
shard_encode_into / compact_merge_into on a context of their own, byte for byte against the oracle --
compact_generate_sst resumed at every carry-in of the grid (carry-out, segments, blocks, the eight stats
words), every error report of the carry and segment kernels with a good call after it, the host-side argument
rules, and the range predicate lo <= key < hi on its edges in every merge mode.  No shard.compact_local: which
branch runs is chosen here, not by a seed."""
import ctypes
import dataclasses
import time

import numpy as np
import pytest
import torch

import path_cases as pc
import shard_cases as sc
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch, shard
from lsm_amd._lib import LSMBLK_ERR_CAPACITY, LSMBLK_ERR_SEGMENTS, LSMBLK_E_INVAL, LsmBlkError
from oracle import oracle as O
from test_gpu_compact import dev_entries, to_dev

pytestmark = pytest.mark.gpu
RUNS, TWO, NEWEST = sc.RUNS, sc.TWO, sc.NEWEST


_memo = {}


def ext_cases():
    if not _memo:
        _memo["cases"] = {c.name: c for c in sc.ext_cases()}
    return _memo["cases"]


class Range:
    """One extended stream on the device with a context of its own and the output buffers of the encode."""

    def __init__(self, case, sst_cap=64, ctx=None):
        self.case, self.sst_cap = case, sst_cap
        self.ctx = ctx if ctx is not None else batch.OwnCtx(torch.cuda.current_device())
        self.d = to_dev(case.ext)
        self.same = torch.from_numpy(case.same).cuda() if case.same is not None else None
        n = case.n
        self.out_cap = int(case.ext.key_off[-1]) + int(case.ext.val_off[-1]) + 18 * n + 16
        self.out = batch._aligned_empty(self.out_cap, "cuda")
        self.blk_cap = n + 2
        self.blk_off = torch.zeros(self.blk_cap, dtype=torch.int64, device="cuda")
        self.seg_cap = max(sst_cap, 2 * n // 3) + 3
        self.seg = torch.zeros(self.seg_cap, dtype=torch.int32, device="cuda")
        self.seg_blk = torch.zeros(self.seg_cap, dtype=torch.int32, device="cuda")
        self.stats = torch.zeros(8, dtype=torch.int64, device="cuda")
        self.cout = torch.zeros(2, dtype=torch.int64, device="cuda")

    def prepare(self):
        c = self.case
        batch.shard_prepare(self.d, c.m, c.last, c.bs, c.target, self.sst_cap, ctx=self.ctx, ext_same=self.same)
        return self

    def carry(self, cin):
        batch.shard_carry(cin, self.cout, ctx=self.ctx)

    def encode(self, seg_cap=None, **kw):
        a = dict(ext=self.d, out=self.out, out_cap=self.out_cap, blk_off=self.blk_off, blk_cap=self.blk_cap,
                 seg_start=self.seg, seg_blk=self.seg_blk, seg_cap=seg_cap or self.seg_cap, stats=self.stats)
        a.update(kw)
        self.seg.fill_(-1)
        batch.shard_encode_into(a["ext"], a["out"], a["out_cap"], a["blk_off"], a["blk_cap"], a["seg_start"], a["seg_blk"],
                                a["seg_cap"], a["stats"], ctx=self.ctx)

    def run(self, cin, seg_cap=None):
        """carry + encode at the device carry-in `cin` -> (carry-out, stats, seg_start, seg_blk, blk_off, blocks)."""
        self.carry(cin)
        self.encode(seg_cap)
        torch.cuda.synchronize()
        s = self.stats.cpu().tolist()
        return (self.cout.cpu().tolist(), s, self.seg.cpu().numpy().view(np.uint32), self.seg_blk.cpu().numpy().view(np.uint32),
                self.blk_off[:s[0] + 1].cpu().numpy().view(np.uint64), self.out[:s[1]].cpu().numpy().tobytes())


def carry_in(p, d0):
    return torch.tensor([p, d0], dtype=torch.int64, device="cuda")


def check_point(case, p, d0, got, ans=None):
    """One carry-in against compact_generate_sst resumed there: carry-out, seg_start, seg_blk, the blocks and
    blk_off (O.encode_span over the oracle's segments) and the eight stats words."""
    cout, s, seg_got, segblk_got, off_got, blocks_got = got
    rc, seg, (p_out, d_out) = ans if ans is not None else sc.oracle_answer(case, p, d0)
    assert rc == O.ORC_OK
    at = (case.name, p, d0)
    assert cout == [p_out, d_out], at
    nseg = max(len(seg) - 1, 0)
    rc, blocks, off = O.encode_span(case.ext, seg, case.bs)
    assert rc == 0
    assert s == [len(off) - 1, len(blocks), nseg, 0, int(nseg > 0 and d0 > 0), int(nseg > 0 and d_out > 0), p, case.m + p_out], at
    assert blocks_got == blocks.tobytes(), at
    np.testing.assert_array_equal(off_got, off, str(at))
    if nseg:
        np.testing.assert_array_equal(seg_got[:nseg + 1], seg, str(at))
        first = np.concatenate([[0], np.cumsum(pc.block_entry_counts(blocks, off.astype(np.int64)))])   # every block's first entry
        blk = np.searchsorted(first, seg.astype(np.int64) - int(seg[0]))
        assert (first[blk] == seg.astype(np.int64) - int(seg[0])).all()   # (no block crosses a segment start)
        np.testing.assert_array_equal(segblk_got[:nseg + 1], blk, str(at))
    return nseg


# ---------------------------------------------------------------- a. the carry sweep
@pytest.mark.parametrize("name", [c.name for c in sc.ext_cases()])
def test_every_carry_in_of_the_grid_equals_the_resumed_oracle(name):
    """One prepare, then carry + encode at every (p, D0) of the grid: the rotation state stays on the context
    however many carries and encodes follow (include/lsmblk.h).  The `ex` streams go through prepare_ex with
    their own same_as_last_key."""
    case = ext_cases()[name]
    r = Range(case).prepare()
    grid = sc.carry_grid(case)
    cins = torch.tensor(grid, dtype=torch.int64, device="cuda")
    t0, seen, counts = time.perf_counter(), set(), set()
    for i, (p, d0) in enumerate(grid):
        ans = sc.oracle_answer(case, p, d0)
        check_point(case, p, d0, r.run(cins[i]), ans)
        labels, cnt = sc.classify(case, p, d0, ans)
        seen |= labels
        counts.add(cnt)
    print(f"{name}: m {case.m}, n {case.n}, block_size {case.bs}, target {case.target}, {'LAST' if case.last else 'no LAST'}: "
          f"{len(grid)} carry-ins in {time.perf_counter() - t0:.2f} s, {sorted(seen)}, SSTs starting in the range "
          f"{sorted(c for c in counts if c is not None)}")


# ---------------------------------------------------------------- b. the error contract
def good_case():
    return ext_cases()["bs256-l1-mid"]


def check_good_call(ctx):
    """After a refused call: prepare, carry and encode of a valid range on the same context equal the oracle (no
    state of the refused call is left)."""
    case = good_case()
    r = Range(case, ctx=ctx).prepare()
    for p, d0 in ((0, 0), (case.m // 2, case.target), (case.m - 1, 1)):
        assert check_point(case, p, d0, r.run(carry_in(p, d0))) > 0


def check_refused(r, p, d0, flag):
    cout, s, seg, _, _, blocks = r.run(carry_in(p, d0))
    assert s[3] == flag and s[:3] == [0, 0, 0] and blocks == b"", (r.case.name, s)
    assert batch._status(r.stats) != 0


@pytest.mark.parametrize("name", ["m_inside_versions", "halo_short", "no_halo_open", "no_halo_reached"])
def test_segments_is_reported(name):
    """LSMBLK_ERR_SEGMENTS: a range that ends inside a key's versions; a halo shorter than the crossing block
    without LAST; and no halo at all without LAST (n == m, p < m), where the carry kernel used to report success
    with carry-out {0, 0} -- with the open SST below its target and with a chain of SSTs that reached theirs.
    The same ext with LAST is valid and equals the oracle."""
    case, p, d0 = sc.error_cases()[name]
    r = Range(case).prepare()
    check_refused(r, p, d0, LSMBLK_ERR_SEGMENTS)
    check_good_call(r.ctx)
    if name != "m_inside_versions":
        last = dataclasses.replace(case, last=True)
        r = Range(last, ctx=r.ctx).prepare()
        assert check_point(last, p, d0, r.run(carry_in(p, d0))) > 0
        assert r.cout.cpu().tolist() == [case.n - case.m, 0]


@pytest.mark.parametrize("c", sc.SST_COUNTS[1:])
def test_sst_cap_covers_the_range_or_capacity_is_reported(c):
    """A range in which c SSTs start: sst_cap == c succeeds, an sst_cap whose 2^shard_flevels lies below c
    reports LSMBLK_ERR_CAPACITY, and any sst_cap between them does one or the other -- never other segments."""
    case = ext_cases()["bs64-l1-mid"]
    answers = {(case.name, p, case.target): sc.oracle_answer(case, p, case.target) for p in range(case.m)}
    p, d0 = sc.sst_count_points(case, answers)[c], case.target
    ctx = batch.OwnCtx(torch.cuda.current_device())
    outcome = {}
    for cap in range(1, c + 1):
        r = Range(case, sst_cap=cap, ctx=ctx).prepare()
        got = r.run(carry_in(p, d0))
        if got[1][3] == 0:
            assert check_point(case, p, d0, got, answers[(case.name, p, d0)]) == c + 1
            outcome[cap] = "ok"
        else:
            assert got[1][3] == LSMBLK_ERR_CAPACITY and got[1][:3] == [0, 0, 0] and got[5] == b"", (cap, got[1])
            outcome[cap] = "capacity"
            check_good_call(ctx)
        if 2 ** sc.shard_flevels(cap) < c:
            assert outcome[cap] == "capacity", (cap, outcome)
    assert outcome[c] == "ok", outcome
    print(f"{c} SSTs start in the range (p {p}): sst_cap -> {outcome}")


def test_seg_cap_one_short_reports_capacity():
    """shard_seg_kernel: seg_cap == nseg + 1 holds the segments; seg_cap == nseg reports LSMBLK_ERR_CAPACITY with
    zero blocks, bytes and segments and every seg_start equal to the end entry -- and the same carry-in right
    after it with room for the segments (same prepare) equals the oracle."""
    case = ext_cases()["bs64-l1-mid"]
    r = Range(case).prepare()
    p, d0 = 3, case.target
    rc, seg, (p_out, _) = sc.oracle_answer(case, p, d0)
    nseg = len(seg) - 1
    assert nseg >= 5
    assert check_point(case, p, d0, r.run(carry_in(p, d0), seg_cap=nseg + 1)) == nseg
    cout, s, seg_got, _, _, blocks = r.run(carry_in(p, d0), seg_cap=nseg)
    assert s[3] == LSMBLK_ERR_CAPACITY and s[:3] == [0, 0, 0] and blocks == b"", s
    assert (seg_got[:nseg] == case.m + p_out).all() and (seg_got[nseg:] == 0xFFFFFFFF).all(), seg_got[:nseg + 2]
    assert check_point(case, p, d0, r.run(carry_in(p, d0))) == nseg   # (the carry clears the report)
    check_good_call(r.ctx)


def status_of(fn):
    with pytest.raises(LsmBlkError) as e:
        fn()
    return e.value.status


def test_host_side_argument_rules():
    """LSMBLK_E_INVAL from the host: carry or encode before any prepare, an ext of another length than the
    prepared one, seg_cap < 2, blk_cap == 0, a misaligned out -- and after each the prepared state still
    serves a carry and an encode."""
    case = good_case()
    r = Range(case)
    assert status_of(lambda: r.carry(carry_in(0, 0))) == LSMBLK_E_INVAL
    assert status_of(lambda: r.encode()) == LSMBLK_E_INVAL
    r.prepare()
    shorter = batch.KVStream(r.d.keys, r.d.key_off, r.d.vals, r.d.val_off, r.d.ts, case.n - 1)
    for kw in (dict(ext=shorter), dict(seg_cap=1), dict(blk_cap=0), dict(out=r.out[1:], out_cap=r.out_cap - 1)):
        r.carry(carry_in(0, 0))
        assert status_of(lambda: r.encode(**kw)) == LSMBLK_E_INVAL, kw
        check_point(case, 5, 1, r.run(carry_in(5, 1)))   # (no new prepare)
    check_good_call(r.ctx)


def test_merge_argument_rules():
    """LSMBLK_E_INVAL from the host: a two_end above LSMBLK_TWO_END_BELOW, a two-level merge without kept_same,
    and any mode but LSMBLK_MERGE_RUNS through lsmblk_compact_merge_batch (the form without _ex)."""
    case = sc.bound_runs()
    m = Merge(case)
    for mode in (RUNS, TWO, NEWEST):
        assert status_of(lambda: m.call(mode, None, None, False, two_end=3)) == LSMBLK_E_INVAL
    assert status_of(lambda: m.call(TWO, None, None, False, kept_same=False)) == LSMBLK_E_INVAL
    want = sc.kept_entries(case, RUNS, False)
    assert m.call(RUNS, None, None, False, plain=True)[0] == want
    for mode in (TWO, NEWEST, 3):
        assert status_of(lambda: m.call(mode, None, None, False, plain=True)) == LSMBLK_E_INVAL
    assert m.call(RUNS, None, None, False)[0] == want   # the context still merges


# ---------------------------------------------------------------- c. range bounds
class Merge:
    """lsmblk_compact_merge_batch[_ex] over the bound runs on a context of its own."""

    def __init__(self, case):
        self.case = case
        self.ctx = batch.OwnCtx(torch.cuda.current_device())
        self.d = to_dev(case.kv)
        self.rt = batch._u32_table(case.rs, torch.device("cuda"))
        kv = case.kv
        self.kept = batch.KVStream.empty(kv.n, int(kv.key_off[-1]), int(kv.val_off[-1]), torch.device("cuda"))
        self.ks = torch.zeros(kv.n + 1, dtype=torch.uint8, device="cuda")
        self.stats = torch.zeros(5, dtype=torch.int64, device="cuda")

    def call(self, mode, lo, hi, bottom, two_end=0, kept_same=True, plain=False):
        """-> (kept entries, stats[0..4], key_off[0], val_off[0])."""
        bound = lambda b: None if b is None else torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8)[:len(b)].cuda()
        lo_t, hi_t = bound(lo), bound(hi)
        rng = batch.key_range_c(lo_t, hi_t) if (lo is not None or hi is not None) else None
        opts = batch.compact_opts(sc.WM, bottom, block_size=4096, target_sst_size=1 << 20, merge_mode=mode)
        self.kept.key_off.fill_(-1)
        self.kept.val_off.fill_(-1)
        self.stats.fill_(-1)
        if plain:
            dev = torch.cuda.current_device()
            o, ci, ck = batch._opts_c(opts), self.d._c(), self.kept._c(*self.kept.caps())
            batch._native("lsmblk_compact_merge_batch", dev, None, ctypes.byref(ci), self.rt.data_ptr(), self.rt.numel() - 1,
                          ctypes.byref(o), ctypes.byref(rng) if rng is not None else None, ctypes.byref(ck),
                          self.stats.data_ptr(), batch._stream_ptr(None, dev), own=self.ctx)
        else:
            batch.compact_merge_into(self.d, self.rt, self.rt.numel() - 1, opts, rng, self.kept, self.stats, ctx=self.ctx,
                                     two_end=two_end, kept_same=self.ks if (mode == TWO and kept_same) else None)
        torch.cuda.synchronize()
        s = self.stats.cpu().tolist()
        k = self.kept
        got = dev_entries(batch.KVStream(k.keys, k.key_off, k.vals, k.val_off, k.ts, s[0])) if s[3] == 0 and s[0] > 0 else []
        return got, s, int(k.key_off[0]), int(k.val_off[0])


MODES = [(RUNS, "runs"), (NEWEST, "newest"), (TWO, "two-level")]


def check_range(m, mode, lo, hi, bottom, kept_all, kb):
    """One (lo, hi) in one mode: the kept entries are the unrestricted kept stream filtered by lo <= key < hi on
    the host; stats[0..2] are their count and bytes, stats[4] the merged count over the whole input (two-level: as
    the range's two_end words it, sc.merged_entries)."""
    case = m.case
    two_end = shard.two_end_mode(kb, lo, hi) if mode == TWO else 0
    want = [e for e in kept_all if sc.in_bounds(e[0], lo, hi)]
    got, s, ko0, vo0 = m.call(mode, lo, hi, bottom, two_end=two_end)
    at = (mode, lo, hi, bottom, two_end)
    assert s[3] == 0 and got == want, at
    merged = len(sc.merged_entries(case, mode, two_end))
    assert s == [len(want), sum(len(e[0]) for e in want), sum(len(e[2]) for e in want), 0, merged], at
    assert (ko0, vo0) == (0, 0), at   # (written for an empty range too)
    return want, merged, two_end


@pytest.mark.parametrize("bottom", [False, True])
@pytest.mark.parametrize("mode,mode_name", MODES)
def test_range_bounds_on_their_edges(mode, mode_name, bottom):
    case = sc.bound_runs()
    sc.check_bound_cases(case)
    m = Merge(case)
    kept_all = sc.kept_entries(case, mode, bottom)
    kb = case.runs()[-1][-1][0]
    sizes, ends = {}, set()
    for name, lo, hi in sc.bound_pairs(case):
        want, merged, two_end = check_range(m, mode, lo, hi, bottom, kept_all, kb)
        sizes[name] = (len(want), merged)
        ends.add(two_end)
    assert sizes["unbounded"][0] == len(kept_all) == sizes["zero-length lo"][0] > 0
    for name in ("zero-length hi", "zero-length lo and hi", "lo equals hi", "lo above hi", "range above every key",
                 "range below every key"):
        assert sizes[name][0] == 0, name
    assert any(0 < k < mg for k, mg in sizes.values())   # stats[4] is not the in-range count
    if mode == TWO:
        assert ends == {0, 1, 2}
        assert sizes["lo just above b's last key"][0] == 0 and sizes["lo at b's last key"][0] > 0
    else:
        assert len({mg for _, mg in sizes.values()}) == 1 and sizes["zero-length hi"][1] > 0
    print(f"{mode_name}, bottom {bottom}: (kept in range, merged) {sizes}")


@pytest.mark.parametrize("mode,mode_name", MODES)
def test_consecutive_ranges_concatenate_to_the_unrestricted_kept_stream(mode, mode_name):
    """Splitters equal to a key, a proper prefix of a key, a key followed by a zero byte, repeated and of zero
    length: the ranges' kept streams in order are the unrestricted kept stream, no entry lost or duplicated."""
    case = sc.bound_runs()
    m = Merge(case)
    kb = case.runs()[-1][-1][0]
    for bottom in (False, True):
        kept_all = sc.kept_entries(case, mode, bottom)
        assert m.call(mode, None, None, bottom, two_end=0)[0] == kept_all
        for sp in sc.splitter_sets():
            parts = [check_range(m, mode, *shard.range_of(r, sp), bottom, kept_all, kb)[0] for r in range(len(sp) + 1)]
            assert [e for p in parts for e in p] == kept_all, (mode_name, bottom, sp)
            assert sum(1 for p in parts if p) >= 4
