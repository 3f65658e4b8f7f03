"""The compaction kernels of lsmblk_compact.hip on every path and on both sides of every
threshold: the inputs of tests/compact_cases.py (derived from the kernels' constants, their
coverage asserted on the CPU by test_compact_cases.py) through the C ABI, bit for bit against the
oracle -- the kept stream's five arrays, the blocks, blk_off, sst_start, sst_blk and the stats
words.  Claimed launch shapes are checked on the context's kernel log.  Run with -s for the coverage."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import compact_cases as cc
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch
from lsm_amd._lib import LSMBLK_E_CAPACITY, LSMBLK_MERGE_RUNS, LSMBLK_MERGE_TWO_LEVEL, kernel_timing
from oracle import oracle as O
from oracle import pyref
from test_gpu_compact import assert_kv_equal, check_compact, check_compact_mode, dev_entries, to_dev

pytestmark = pytest.mark.gpu
RUNS, TWO = LSMBLK_MERGE_RUNS, LSMBLK_MERGE_TWO_LEVEL
C = cc.C


@contextlib.contextmanager
def launches():
    """{kernel: launches} of the calls made inside, from the context's kernel log."""
    with kernel_timing(batch._ctx(torch.cuda.current_device())) as log:
        yield log
    log.update({k: v[0] for k, v in log.items()})


def gpu_merge(d, rs, mode):
    """batch.merge_runs with the stats words: (merged KVStream, stats)."""
    dev = torch.device("cuda")
    rt = batch._u32_table(rs, dev)
    kb, vb = d.byte_sizes()
    out = batch.KVStream.empty(d.n, kb, vb, dev)
    stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device=dev)
    batch.merge_into(d, rt, rt.numel() - 1, out, stats, merge_mode=mode)
    torch.cuda.synchronize()
    s = stats.cpu().tolist()
    assert s[3] == 0, s
    out.n = s[0]
    return out, s


def check_merge(case, two=True, rule=True):
    """Both merge modes against the references: O.merge_runs (and pyref.merge_runs_rule) for the run
    merge, pyref.two_merge_rule for the two-level one; stats = (entries, key bytes, value bytes)."""
    kv, d = case.kv, to_dev(case.kv)
    want = O.gather(kv, O.merge_runs(kv, case.rs))
    got, s = gpu_merge(d, case.rs, RUNS)
    assert_kv_equal(got, want)
    assert s[:3] == [want.n, int(want.key_off[-1]), int(want.val_off[-1])]
    runs = case.runs() if (two or rule) else None
    if rule:
        assert want.entries() == pyref.merge_runs_rule(runs)
    if two:
        want2 = pyref.two_merge_rule(runs)
        got, s = gpu_merge(d, case.rs, TWO)
        assert dev_entries(got) == want2
        assert s[:3] == [len(want2), sum(len(k) for k, _, _ in want2), sum(len(v) for _, _, v in want2)]
    return want


def check_compact_stats(kv, rs, wm, bottom, pf, bs, target):
    """test_gpu_compact.check_compact (kept stream, blocks, blk_off, sst_start, sst_blk against
    O.compact) and the eight stats words."""
    got, want = check_compact(kv, rs, wm, bottom, pf, bs, target)
    kl, vl = cc.merged_lengths(kv, O.merge_runs(kv, rs)[want["kept"]])
    assert got["stats"] == [len(want["blk_off"]) - 1, len(want["blocks"]), len(want["sst_blk"]) - 1, 0,
                            got["stats"][4], len(want["kept"]), int(kl.sum()), int(vl.sum())]
    return got, want


def rotation_raw(d, bs, target, sst_cap):
    """lsmblk_sst_rotation_batch -> (status, stats, starts tensor)."""
    dev = torch.cuda.current_device()
    starts = torch.zeros(sst_cap, dtype=torch.int32, device="cuda")
    stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device="cuda")
    c = d._c()
    batch._native("lsmblk_sst_rotation_batch", dev, None, ctypes.byref(c), bs, target, starts.data_ptr(), sst_cap,
                  stats.data_ptr(), batch._stream_ptr(None, dev))
    torch.cuda.synchronize()
    return batch._status(stats), stats.cpu().tolist(), starts


# ---------------------------------------------------------------- key order
@pytest.mark.parametrize("last", cc.KEY_ORDER_LAST)
def test_key_order_through_the_16_byte_images(last):
    """Zero bytes, zero-extended prefixes, 16-byte keys beside longer ones, tails that first differ
    at byte 1-5, 8, 9 (the partial last dword of key_diff), a 65 535-byte key, and a long
    last key of the arena: merge in both modes, the rules + rotation + blocks (rot_adj through
    kidx / image_lcp), and the stand-alone rotation of the kept stream (rot_adj through key_diff)."""
    case = cc.key_order(last)
    nkeys, nties = cc.check_key_order(case)
    merged = check_merge(case)
    for wm, bottom, pf, bs, target in ((0, False, (), 4096, 1 << 20), (500, True, (b"\0", b"m\x7f", b"q" * 17), 256, 700),
                                       (500, False, (b"\xff",), 64, 1)):
        got, want = check_compact_stats(case.kv, case.rs, wm, bottom, pf, bs, target)
        kept = O.gather(merged, want["kept"])
        np.testing.assert_array_equal(batch.sst_rotation(to_dev(kept), bs, target), want["sst_ent"])
        check_compact_mode(case.runs(), TWO, wm, bottom, pf, bs, target)
    print(f"key-order[{last}]: {nkeys} keys over {len(case.rs) - 1} runs, {nties} shared 16-byte images, "
          f"{case.kv.n} entries -> {merged.n} merged")


def test_lcp_of_zero_padded_images():
    """image_lcp where the 16-byte images first differ past the shorter key's end (a zero pad against
    zero bytes of the longer key): the LCP is the shorter length.  The first SST's end depends on it."""
    case = cc.pad_lcp()
    nsst = cc.check_pad_lcp(case)
    got, want = check_compact_stats(case.kv, case.rs, 0, False, (), cc.CHAIN_BS, 1)
    assert want["sst_ent"][1] == 3 and got["stats"][2] == nsst
    np.testing.assert_array_equal(batch.sst_rotation(to_dev(case.kv), cc.CHAIN_BS, 1), want["sst_ent"])


# ---------------------------------------------------------------- tile size edges
@pytest.mark.parametrize("X", cc.tile_edge_sizes())
def test_merge_tile_size_edges(X):
    """A tile of exactly X entries (kMTE - 1 .. 2 kBigTE + 3): merge_tile_kernel up to kMTE,
    merge_big_kernel up to kBigTE, the one-wave global path beyond; in one run (every entry
    survives: the u16 survivor prefix reaches X) and split over 2, 3 and 64 runs, both modes."""
    seen = []
    for nrun in cc.TILE_NRUN:
        case = cc.tile_edge(X, nrun)
        kern, surv = cc.check_tile_edge(case)
        check_merge(case)
        seen.append((nrun, kern, surv))
    print(f"tile-edge[{X}]: (runs, kernel, survivors) {seen}")


# ---------------------------------------------------------------- tile scan
@pytest.mark.parametrize("nc", cc.tile_scan_ncs())
def test_merge_tile_scan_parts(nc):
    """kTScan, kTScan + 1 and 2 kTScan + 2 tiles: one, two and three parts of tscan_part_kernel,
    tscan_top_kernel's bases and perm_kernel's tbase[t / kTScan]."""
    case = cc.tile_scan(nc)
    got_nc, parts = cc.check_tile_scan(case)
    want = check_merge(case, two=nc == C.kTScan + 1, rule=False)
    print(f"tile-scan[{nc}]: {case.kv.n} entries, {got_nc} tiles in {parts} parts -> {want.n} merged")


# ---------------------------------------------------------------- gather scan
def test_gather_scan_second_part():
    """kGScan kGTile + kGTile + 5 merged entries: mscan_part_kernel's second part, mscan_top_kernel
    and mwrite_kernel's part_pre[3 (blockIdx.x / kGScan)] with non-zero bases of all three sums."""
    case = cc.gather_scan()
    got, want = check_compact_stats(case.kv, case.rs, case.info["wm"], True, (case.info["prefix"],), 4096, 1 << 20)
    tiles, parts, base = cc.check_gather_scan(case, want["kept"])
    assert parts == 2 and base > 0
    print(f"gather-scan: {case.kv.n} entries -> {got['stats'][4]} merged in {tiles} tiles / {parts} parts, "
          f"{len(want['kept'])} kept ({base} before part 1), {got['stats'][6]} key B, {got['stats'][7]} value B")


# ---------------------------------------------------------------- neighbour hand-off
@pytest.mark.parametrize("bottom", [False, True])
@pytest.mark.parametrize("prefix", [False, True])
def test_version_groups_across_round_and_tile_starts(bottom, prefix):
    """Version groups that end at, start at and span merged positions 256 m and kGTile m (thread 0
    of mflag_kernel / rot_adj_kernel loads its predecessor from global memory), timestamps on both
    sides of the watermark, tombstones first: the rules in both merge modes, and the plain merge."""
    case = cc.round_straddle()
    seen = cc.check_round_straddle(case)
    pf = (case.info["prefix"],) if prefix else ()
    wm = case.info["wm"]
    for bs, target in ((4096, 1 << 20), (64, 1)):
        check_compact_stats(case.kv, case.rs, wm, bottom, pf, bs, target)
        check_compact_mode(case.runs(), TWO, wm, bottom, pf, bs, target)
    if not bottom and not prefix:
        check_merge(case, rule=False)   # (pyref.merge_runs_rule is quadratic in the keys)
        print(f"round-straddle: {case.kv.n} entries; (kGTile multiple, kind, predecessor <= wm, entry <= wm) "
              f"{sorted(seen, key=str)}")


# ---------------------------------------------------------------- copy shapes
def test_mwrite_copy_shapes():
    """Key and value lengths over 0, 1, 3, 4, 7, 8, 15, 16, 17, 31, 32, 128, 129, 130, 257, 1000 in
    staged rounds (lds_put's three branches, wave_copy_packed with a second outer pass) and
    unstaged ones (lane_copy, copy16_batched's second batch), every lead, the images filled
    exactly and one byte over, kept and dropped entries interleaved."""
    case = cc.copy_shape()
    wm = case.info["wm"]
    got, want = check_compact_stats(case.kv, case.rs, wm, False, (), 4096, 1 << 20)
    g = cc.check_copy_shape(case, want["kept"])
    print(cc.copy_coverage(g))
    check_compact_stats(case.kv, case.rs, wm, True, (b"\x01",), 1024, 20000)
    check_compact_mode(case.runs(), TWO, wm, False, (), 4096, 1 << 20)
    check_merge(case, rule=False)   # every entry kept: mwrite_kernel<true, true>, other round sums


# ---------------------------------------------------------------- rotation window and levels
_rot = {}


def rot_stream(name):
    if name not in _rot:
        if name == "short":
            _rot[name] = cc.rot_short_keys()
        elif name == "uniform":
            _rot[name] = cc.rot_uniform()
        elif name == "swap-near":
            _rot[name] = cc.swap_pair(rot_stream("uniform"), cc.ROUND + 300)[0]
        elif name == "prefix":
            _rot[name] = cc.rot_prefix_runs()
        elif name == "swap-prefix":
            _rot[name] = cc.swap_pair(rot_stream("prefix"), cc.ROUND + C.kRotWin + 100)[0]
        elif name == "swap-far":
            _rot[name] = cc.swap_pair(rot_stream("short"), 2 * cc.ROUND + C.kRotWin + 50)[0]
    return _rot[name]


@pytest.mark.parametrize("name,bs", [("short", 65536), ("short", 16384), ("uniform", 16384), ("swap-near", 16384),
                                     ("swap-far", 16384), ("swap-far", 65536), ("prefix", 65536), ("prefix", 16384),
                                     ("swap-prefix", 65536)])
def test_rotation_walks_past_the_lds_window(name, bs):
    """Blocks of more than 256 + kRotWin entries (rot_next_kernel reads global memory past its
    window), block ends on every offset around the window's edge (the fast walk's hand-over at
    wend - kRotStep), and one unsorted pair inside the fast walk's range (slow, then direct) or
    past the window; the prefix streams drop the LCP only past the window, so the block's size
    depends on the alcp read there.  The sorted streams also through lsmblk_compact_batch (rot_adj
    by kidx)."""
    kv = rot_stream(name)
    d = to_dev(kv)
    if name == "uniform":
        cc.check_window_edge(kv, bs)
    if name == "prefix":
        cc.check_prefix_runs(kv, bs)
    nsst = []
    for target in (1, 3 * bs, 1 << 40):
        want = O.segment_like_compaction(kv, bs, target)
        np.testing.assert_array_equal(batch.sst_rotation(d, bs, target), want)
        nsst.append(len(want) - 1)
    if not name.startswith("swap"):
        got, want = check_compact_stats(kv, np.array([0, kv.n], np.uint32), 0, False, (), bs, 3 * bs)
        assert got["stats"][5] == kv.n
    cnt = cc.block_counts(kv, [0, kv.n], bs)
    print(f"rotation-window[{name}, {bs}]: {kv.n} entries, blocks of {int(cnt.min())}-{int(cnt.max())} entries, "
          f"SSTs at targets 1 / 3 blocks / 2^40: {nsst}")


@pytest.mark.parametrize("bs,name", [(256, "uniform"), (256, "short")])
def test_rotation_level_counts(bs, name):
    """rot_levels 1..5: level 0 alone (target < kRotHops blocks), then rot_double2_kernel and
    rot_double_kernel by the parity of the level count -- asserted on the launches."""
    kv = rot_stream(name)
    d = to_dev(kv)
    targets = cc.level_targets(bs)
    cc.check_level_targets(targets, bs)
    seen = {}
    for lv, target in targets.items():
        want = O.segment_like_compaction(kv, bs, target)
        with launches() as log:
            got = batch.sst_rotation(d, bs, target)
        np.testing.assert_array_equal(got, want)
        assert (log.get("rot_double2_kernel", 0), log.get("rot_double_kernel", 0)) == cc.rot_double_launches(lv), log
        assert len(want) > 3
        seen[lv] = len(want) - 1
    print(f"rotation-levels[{name}]: block_size {bs}, {{levels: SSTs}} {seen}")


def test_rotation_more_levels_than_needed():
    """A large target over a stream of two blocks: five levels allocated and launched, but after
    level 1 every chain is at the end (cc.check_levels_not_needed: J0[J0[s]] == n), so need[1..]
    stay 0 and the doubling kernels of levels 2..4 return at once; rot_f_kernel's rot_top stops
    at level 1."""
    kv, bs = cc.rot_tiny(), 256
    target = cc.level_targets(bs)[5]
    assert cc.check_levels_not_needed(kv, bs, target) == 5
    want = O.segment_like_compaction(kv, bs, target)
    with launches() as log:
        got = batch.sst_rotation(to_dev(kv), bs, target)
    np.testing.assert_array_equal(got, want)
    assert (log.get("rot_double2_kernel", 0), log.get("rot_double_kernel", 0)) == cc.rot_double_launches(5), log
    got, _ = check_compact_stats(kv, np.array([0, kv.n], np.uint32), 0, False, (), bs, target)
    assert got["stats"][2] == 1


# ---------------------------------------------------------------- SST chain
def chain_kv(n, versions=1):
    key = ("chain", versions)
    if key not in _rot:
        _rot[key] = cc.chain_stream(max(m for m, _, _ in cc.chain_cases()) if versions == 1 else 4 * 6144, versions)
    return cc.prefix_kv(_rot[key], n)


def check_chain(kv, cap, nsst):
    want = O.segment_like_compaction(kv, cc.CHAIN_BS, 1)
    assert len(want) - 1 == nsst
    lc, K, walks, nchain = cc.chain_plan(cap)
    d = to_dev(kv)
    with launches() as log:
        status, stats, starts = rotation_raw(d, cc.CHAIN_BS, 1, cap)
    assert ("rot_walk_kernel" in log, "rot_fill_kernel" in log) == (walks, walks), (log, lc, K)
    assert log["rot_chain_kernel"] == nchain, (log, lc, K)
    if cap >= nsst + 1:
        assert status == 0 and stats[0] == nsst and stats[3] == 0, (status, stats)
        got = starts.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got[:nsst + 1], want)
        assert (got[nsst:] == kv.n).all()
        np.testing.assert_array_equal(batch.sst_rotation(d, cc.CHAIN_BS, 1, sst_cap=cap), want)
    else:   # the chain does not end in the array: status and stats only
        assert status == LSMBLK_E_CAPACITY and stats[0] == cap == nsst, (status, stats)
        with pytest.raises(batch.LsmBlkError) as e:
            batch.sst_rotation(d, cc.CHAIN_BS, 1, sst_cap=cap)
        assert e.value.status == LSMBLK_E_CAPACITY
    return lc, K, walks


@pytest.mark.parametrize("n,cap,nsst", cc.chain_cases())
def test_sst_chain_fills_the_array(n, cap, nsst):
    """One SST per two entries (64-byte blocks, target 1) in an array that the chain fills exactly
    (sst_cap = nsst + 1) or overflows by one: lc of cc.chain_lcs, i.e. K = 3, 4, 5, 7, 8 doubling levels
    with walk + fill, and full doubling; 2^3 and 2^3 + 1 slots around the last level's squaring."""
    lc, K, walks = check_chain(chain_kv(n), cap, nsst)
    print(f"chain[{n}, {cap}]: {nsst} SSTs, lc {lc}, K {K}, walk + fill {walks}, "
          f"{'fits' if cap > nsst else 'LSMBLK_E_CAPACITY'}")


@pytest.mark.parametrize("cap", [6145, 6144, 9000])
def test_sst_chain_steps_over_same_key_runs(cap):
    """Four versions per key: key_change_after steps over the same-key entries at every SST end."""
    check_chain(chain_kv(4 * 6144, versions=4), cap, 6144)
