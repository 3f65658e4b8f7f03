"""The compaction inputs of tests/compact_cases.py, checked on the CPU: every generator must reach
the tile sizes, scan parts, copy shapes, walks, level counts and chain plans it was built for, and
fail those checks against other constants; and the two references (the C oracle and the
line-by-line oracle/pyref.py) must agree on zero bytes and long key tails before the GPU is held
to them.  test_gpu_compact_paths.py runs the same inputs on the device."""
import dataclasses

import numpy as np
import pytest

import compact_cases as cc
from oracle import oracle as O
from oracle import pyref


def other(**kw):
    return dataclasses.replace(cc.C, **kw)


def test_constants_are_read_from_the_kernel_source(tmp_path):
    c = cc.C
    assert c.kMTE < c.kBigTE < (1 << 16) and c.kMS <= c.kMTE and c.kGTile % cc.ROUND == 0
    assert c.kGKImg % 16 == 0 and c.kGVImg % 16 == 0 and c.kRotStep < c.kRotWin and c.kRotFillMax >= 3
    text = open(cc._SRC).read()
    f = tmp_path / "k.hip"
    mte, tscan = f"#define LSMBLK_MTE {c.kMTE}\n", f"constexpr uint32_t kTScan = {c.kTScan};"
    assert mte in text and tscan in text
    f.write_text(text.replace(mte, f"#define LSMBLK_MTE {c.kMTE + 128}\n")
                 .replace(tscan, f"constexpr uint32_t kTScan = {c.kTScan // 2};"))
    c2 = cc.kernel_constants(str(f))
    assert (c2.kMTE, c2.kTScan) == (c.kMTE + 128, c.kTScan // 2) and c2.kMS == c.kMS
    for gone in ("constexpr uint32_t kGScan = ", "#define LSMBLK_MS "):
        assert gone in text
        f.write_text(text.replace(gone, gone.replace("kGScan", "kGScanX").replace("LSMBLK_MS", "LSMBLK_MSX")))
        with pytest.raises(RuntimeError):
            cc.kernel_constants(str(f))


def test_key_order_streams_tie_on_the_16_byte_images():
    for last in cc.KEY_ORDER_LAST:
        case = cc.key_order(last)
        nkeys, nties = cc.check_key_order(case)
        assert 3 <= len(case.rs) - 1 <= 5
    print(f"key-order: {nkeys} keys, {nties} shared 16-byte images, {case.kv.n} entries")


def test_tile_edges_sit_on_both_sides_of_the_limits():
    seen = {}
    for X in cc.tile_edge_sizes():
        for nrun in cc.TILE_NRUN:
            kern, surv = cc.check_tile_edge(cc.tile_edge(X, nrun))
            seen[(X, nrun)] = (kern, surv)
    c = cc.C
    assert [seen[(X, 1)][0] for X in cc.tile_edge_sizes()] == ["tile", "tile", "big", "big", "big", "global", "global"]
    assert seen[(c.kBigTE, 1)] == ("big", c.kBigTE)   # the u16 survivor prefix at its largest value
    print("tile-edge:", {k: v for k, v in seen.items() if k[1] in (1, 64)})
    # built for other constants the probes leave the edges, and the checks notice
    for c2 in (other(kMTE=c.kMTE + 128), other(kBigTE=c.kBigTE - 512)):
        with pytest.raises(AssertionError):
            for X in cc.tile_edge_sizes():
                cc.check_tile_edge(cc.tile_edge(X, 2), c2)
        for X in cc.tile_edge_sizes(c2):
            cc.check_tile_edge(cc.tile_edge(X, 2, c2), c2)   # the probes follow the constant


def test_tile_scan_candidate_counts():
    c = cc.C
    got = [cc.check_tile_scan(cc.tile_scan(nc)) for nc in cc.tile_scan_ncs()]
    assert got == [(c.kTScan, 1), (c.kTScan + 1, 2), (2 * c.kTScan + 2, 3)]
    case = cc.tile_scan(c.kTScan + 1)
    for c2 in (other(kTScan=c.kTScan // 2), other(kMS=c.kMS * 2)):
        with pytest.raises(AssertionError):
            cc.check_tile_scan(case, c2)
    c2 = other(kTScan=c.kTScan // 2)
    assert cc.check_tile_scan(cc.tile_scan(c2.kTScan + 1, c2), c2) == (c2.kTScan + 1, 2)
    print("tile-scan: NC, parts", got)


def test_gather_scan_starts_a_second_part():
    c = cc.C
    case = cc.gather_scan()
    src = O.merge_runs(case.kv, case.rs)
    assert len(src) == case.info["M"] == c.kGScan * c.kGTile + c.kGTile + 5
    kept = O.compact(case.kv, src, case.info["wm"], True, (case.info["prefix"],), 4096, 1 << 20, kept_only=True)["kept"]
    tiles, parts, base = cc.check_gather_scan(case, kept)
    assert parts == 2 and base > 0
    pf = [i for i in range(0, len(src), 4099) if case.kv.entry(int(src[i]))[0].startswith(case.info["prefix"])]
    assert pf
    with pytest.raises(AssertionError):
        cc.check_gather_scan(case, kept, other(kGScan=c.kGScan * 2))
    with pytest.raises(AssertionError):
        cc.check_gather_scan(case, kept, other(kGTile=c.kGTile // 2))
    print(f"gather-scan: {len(src)} merged, {len(kept)} kept, {tiles} tiles in {parts} parts, part 1 base {base}")


def test_round_straddle_positions_fall_on_the_multiples():
    case = cc.round_straddle()
    seen = cc.check_round_straddle(case)
    with pytest.raises(AssertionError):
        cc.check_round_straddle(case, other(kGTile=4 * cc.C.kGTile))   # too few of its multiples in the stream
    c2 = other(kGTile=2 * cc.C.kGTile)
    cc.check_round_straddle(cc.round_straddle(c2), c2)
    print("round-straddle:", sorted(seen, key=str))


def test_copy_shape_rounds():
    c = cc.C
    case = cc.copy_shape()
    src = O.merge_runs(case.kv, case.rs)
    assert (src == np.arange(case.kv.n)).all()
    kept = O.compact(case.kv, src, case.info["wm"], False, (), 4096, 1 << 20, kept_only=True)["kept"]
    g = cc.check_copy_shape(case, kept)
    print(cc.copy_coverage(g))
    allk = np.arange(case.kv.n)
    print("keep-all (merge):", cc.copy_coverage(cc.gather_rounds(*cc.merged_lengths(case.kv, allk), np.ones(case.kv.n, bool))))
    for c2 in (other(kGKImg=c.kGKImg + 16), other(kGVImg=c.kGVImg - 16), other(kCopyB=c.kCopyB * 2)):
        with pytest.raises(AssertionError):
            cc.check_copy_shape(case, kept, c2)
        case2 = cc.copy_shape(c2)
        kept2 = O.compact(case2.kv, np.arange(case2.kv.n, dtype=np.uint32), case2.info["wm"], False, (), 4096, 1 << 20,
                          kept_only=True)["kept"]
        cc.check_copy_shape(case2, kept2, c2)


def test_rotation_window_streams():
    c = cc.C
    kv = cc.rot_short_keys()
    for bs in (65536, 16384):
        cnt = cc.block_counts(kv, [0, kv.n], bs)
        assert cnt[:-1].min() > cc.ROUND + c.kRotWin, cnt
        print(f"rotation-window: {kv.n} entries, block_size {bs}: blocks of {cnt.tolist()} entries")
    uni = cc.rot_uniform()
    found = cc.check_window_edge(uni, 16384)
    print("window edge offsets -> starts:", found)
    with pytest.raises(AssertionError):
        cc.check_window_edge(uni, 16384, other(kRotWin=c.kRotWin // 2))
    with pytest.raises(AssertionError):
        cc.check_window_edge(uni, 16384, other(kRotWin=c.kRotWin * 2))
    # the unsorted pairs: inside the fast walk's range of workgroup 1, and past its window
    sw, q = cc.swap_pair(uni, cc.ROUND + 300)
    assert q + 1 + c.kRotStep <= cc.ROUND + cc.ROUND + c.kRotWin and cc.block_end(uni, cc.ROUND, 16384) > q + 1
    far, q = cc.swap_pair(kv, cc.ROUND + cc.ROUND + c.kRotWin + 50)
    assert q >= 2 * cc.ROUND + c.kRotWin and cc.block_end(kv, cc.ROUND + 100, 16384) > q + 1
    pre = cc.rot_prefix_runs()
    print("prefix runs: first start crossing a prefix change past the window:",
          {bs: cc.check_prefix_runs(pre, bs) for bs in (65536, 16384)})
    with pytest.raises(AssertionError):
        cc.check_prefix_runs(pre, 16384, other(kRotWin=4 * c.kRotWin))
    assert cc.check_pad_lcp(cc.pad_lcp()) > 4
    for bs in (256, 16384):
        t = cc.level_targets(bs)
        cc.check_level_targets(t, bs)
        with pytest.raises(AssertionError):
            cc.check_level_targets(t, bs, other(kRotHops=c.kRotHops * 2))
    tiny, t5 = cc.rot_tiny(), cc.level_targets(256)[5]
    assert cc.check_levels_not_needed(tiny, 256, t5) == 5
    with pytest.raises(AssertionError):   # 700 entries: chains short of the end at every level
        cc.check_levels_not_needed(cc.prefix_kv(uni, 700), 256, t5)
    assert [cc.rot_double_launches(lv) for lv in range(1, 6)] == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)]


def test_chain_cases_reach_every_k():
    c = cc.C
    cases = cc.chain_cases()
    ks = cc.check_chain_cases(cases)
    with pytest.raises(AssertionError):
        cc.check_chain_cases(cases, other(kRotFillMax=c.kRotFillMax - 1))
    c2 = other(kRotFillMax=c.kRotFillMax - 1)
    cc.check_chain_cases(cc.chain_cases(c2), c2)   # the probes follow the constant
    kv = cc.chain_stream(max(n for n, _, _ in cases))
    for n, cap, nsst in cases:
        if n <= 1 << 14:
            assert len(O.segment_like_compaction(cc.prefix_kv(kv, n), cc.CHAIN_BS, 1)) - 1 == nsst
    assert cc.chain_plan(8)[2] is False and cc.chain_plan(9)[2] is True   # the (2 << k) < sst_cap edge
    v4 = cc.chain_stream(4 * 6144, versions=4)
    want = O.segment_like_compaction(v4, cc.CHAIN_BS, 1)
    assert len(want) - 1 == 6144 and (np.diff(want.astype(np.int64)) == 4).all()
    print("chain (lc, K, walk + fill, fits):", sorted(ks, key=str))


# ------------------------------------------------------------------- the two references agree
def pyref_compact(runs, wm, bottom, pf, bs, target):
    try:
        return pyref.compact_generate_sst(pyref.MergeIterator([pyref.ListIter(r) for r in runs]), wm, bottom, pf, bs,
                                          target)
    except AssertionError:   # the reference panics building an empty SST: nothing may be kept then
        return None


@pytest.mark.parametrize("which", ["key-order-1", "key-order-2", "key-order-3", "copy-shape"])
def test_c_oracle_agrees_with_the_line_by_line_restatement(which):
    """O.merge_runs / O.compact / O.segment_like_compaction against oracle/pyref.py on the key-order
    streams (zero bytes, zero-extended prefixes, long tails, a 65 535-byte key) and on a shrunk
    copy-shape stream (every length class, dropped entries between kept ones)."""
    if which == "copy-shape":
        case, opts = cc.copy_shape(nlead=1), [(100, False, (), 4096, 30000), (100, True, (b"\0\0",), 1024, 5000)]
    else:
        case = cc.key_order(int(which[-1]))
        opts = [(0, False, (), 4096, 1 << 20), (500, True, (b"\0", b"m\x7f", b"q" * 17), 256, 700),
                (500, False, (b"\xff",), 64, 1)]
    runs, kv = case.runs(), case.kv
    src = O.merge_runs(kv, case.rs)
    merged = [kv.entry(int(i)) for i in src]
    assert merged == pyref.merge_runs(runs) == pyref.merge_runs_rule(runs)
    assert pyref.two_merge_runs(runs) == pyref.two_merge_rule(runs)
    for wm, bottom, pf, bs, target in opts:
        want = pyref_compact(runs, wm, bottom, pf, bs, target)
        got = O.compact(kv, src, wm, bottom, pf, bs, target)
        if want is None:
            assert len(got["kept"]) == 0 and len(got["blocks"]) == 0
            continue
        kept = O.gather(kv, src[got["kept"]])
        assert kept.entries() == [e for _, es in want for e in es]
        assert got["blocks"].tobytes() == b"".join(b for sst, _ in want for b in sst)
        assert np.diff(got["sst_ent"].astype(np.int64)).tolist() == [len(e) for _, e in want]
        assert np.diff(got["sst_blk"].astype(np.int64)).tolist() == [len(s) for s, _ in want]
        np.testing.assert_array_equal(O.segment_like_compaction(kept, bs, target), got["sst_ent"])
