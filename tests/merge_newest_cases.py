"""Inputs and expectations for the snapshot-preserving merge (LSMBLK_MERGE_NEWEST) -- TEST INFRASTRUCTURE.

The method of compact_cases.py for the third merge mode of lsmblk_compact.hip; shared by
test_merge_newest_cases.py (CPU: two independent routes to every expected order, and the generators
reach what they were built for) and test_gpu_merge_newest.py (GPU: every byte against the oracle).

  expected order   newest_order(): a stable sort of every entry by (key, -ts, run, position);
                   heap_order(): a heap merge of the runs on (key, Reverse(ts), run), line by line
  expected output  O.compact(kv, src=<that order>, ...): the oracle's own compact_generate_sst loop
                   over the newest-order stream
  snapshot reads   snapshot_rows(): per key the newest version at or below T, a tombstone hides
  generators       run sets, each the smallest shape that reaches its path, sized from the kernels'
                   constants (compact_cases.C); the check_* functions take the constants they check
                   against, so a case built for other constants fails them
"""
import heapq

import numpy as np

import compact_cases as cc
import path_cases as pc
from oracle import oracle as O

C = cc.C
U64 = (1 << 64) - 1
NEWEST = 2  # LSMBLK_MERGE_NEWEST


# ------------------------------------------------------------------------------ expected order
def newest_order(case):
    """Route (a): input indices in (key, ts descending, run, position) order, by a stable sort."""
    tagged, g = [], 0
    for r, run in enumerate(case.runs()):
        for pos, (k, ts, _) in enumerate(run):
            tagged.append((k, -ts, r, pos, g))
            g += 1
    return np.array([x[4] for x in sorted(tagged)], np.uint32)


def heap_order(case):
    """Route (b): a heap merge of the runs on (key, Reverse(ts), run); next() advances the popped
    run alone, never another run's equal key."""
    runs, rs = case.runs(), case.rs.astype(np.int64)
    heap = [(run[0][0], -run[0][1], r) for r, run in enumerate(runs) if run]
    heapq.heapify(heap)
    at, out = [0] * len(runs), []
    while heap:
        _, _, r = heapq.heappop(heap)
        out.append(int(rs[r]) + at[r])
        at[r] += 1
        if at[r] < len(runs[r]):
            k, ts, _ = runs[r][at[r]]
            heapq.heappush(heap, (k, -ts, r))
    return np.array(out, np.uint32)


def runs_in_order(case):
    """The precondition: every run in (key ascending, ts descending) order, no (key, ts) twice."""
    return all((a[0], -a[1]) < (b[0], -b[1]) for run in case.runs() for a, b in zip(run, run[1:]))


def multi_run_keys(case):
    """Keys that live in two or more runs."""
    seen, multi = {}, set()
    for r, run in enumerate(case.runs()):
        for k, _, _ in run:
            if seen.setdefault(k, r) != r:
                multi.add(k)
    return multi


def run_of(case, idx):
    """The run of every input index."""
    return np.searchsorted(case.rs.astype(np.int64), np.asarray(idx, np.int64), "right") - 1


def expected_compact(case, wm, bottom, prefixes, bs, target, order=None):
    """(src, the oracle's compact_generate_sst over kv[src])."""
    src = newest_order(case) if order is None else order
    return src, O.compact(case.kv, src, wm, bottom, prefixes, bs, target)


def snapshot_rows(entries, T):
    """What a snapshot reader at T sees of a set of entries (any order): per key its newest
    version at or below T -- on an equal ts the first in `entries` -- unless that is a tombstone."""
    best = {}
    for k, ts, v in entries:
        if ts <= T and (k not in best or ts > best[k][1]):
            best[k] = (k, ts, v)
    return [e for _, e in sorted(best.items()) if e[2]]


# ------------------------------------------------------------------------------ versions over runs
def interleaved():
    """k-inter's ts interleaved over three runs (run 0: 9, 4; run 1: 7, 6, 1; run 2: 8, 5; run 1's
    6 a tombstone), m-two as an L0 table over a level (run 0: 9; run 1: 5, 3), t-tomb's tombstone
    the overall newest version in run 1 over run 0's value, u-tomb's tombstone the newest of run 0
    only, keys of one run on both sides."""
    v = lambda r, ts: b"r%d@%d" % (r, ts)
    r0 = [(b"a-only", 5, b"a5"), (b"k-inter", 9, v(0, 9)), (b"k-inter", 4, v(0, 4)), (b"m-two", 9, v(0, 9)),
          (b"t-tomb", 3, v(0, 3)), (b"u-tomb", 4, b"")]
    r1 = [(b"b-only", 7, b"b7"), (b"b-only", 2, b"b2"), (b"k-inter", 7, v(1, 7)), (b"k-inter", 6, b""), (b"k-inter", 1, v(1, 1)),
          (b"m-two", 5, v(1, 5)), (b"m-two", 3, v(1, 3)), (b"t-tomb", 8, b""), (b"u-tomb", 7, v(1, 7))]
    r2 = [(b"k-inter", 8, v(2, 8)), (b"k-inter", 5, v(2, 5)), (b"z-last", 2, b"z2")]
    return cc.case_of_runs([r0, r1, r2], hot=b"k-inter")


def check_interleaved(case):
    src = newest_order(case)
    hot = [(int(run_of(case, [i])[0]), case.kv.entry(int(i))[1]) for i in src if case.kv.entry(int(i))[0] == case.info["hot"]]
    assert [ts for _, ts in hot] == [9, 8, 7, 6, 5, 4, 1] and [r for r, _ in hot] == [0, 2, 1, 1, 2, 0, 1]
    return hot


def equal_ts():
    """e-equal holds ts 4 in three runs, each with its own value (run order decides), between
    versions that interleave; f-equal the same with the largest ts."""
    r0 = [(b"e-equal", 7, b"e0.7"), (b"e-equal", 4, b"e0.4"), (b"e-equal", 2, b"e0.2"), (b"f-equal", U64, b"f0")]
    r1 = [(b"e-equal", 4, b"e1.4"), (b"e-equal", 3, b"e1.3"), (b"f-equal", U64, b""), (b"f-equal", 5, b"f1.5")]
    r2 = [(b"e-equal", 9, b"e2.9"), (b"e-equal", 4, b"e2.4"), (b"e-equal", 1, b"e2.1"), (b"f-equal", U64, b"f2")]
    return cc.case_of_runs([r0, r1, r2])


def u64_edges():
    """ts 0, 1, 2^63 - 1, 2^63 and 2^64 - 1 on one key across three runs (and a second key with the
    runs exchanged): a signed compare orders 2^63 and 2^64 - 1 below 0."""
    H = 1 << 63
    r0 = [(b"s-edge", H, b"h"), (b"s-edge", 0, b"0"), (b"t-edge", H - 1, b"h-1")]
    r1 = [(b"s-edge", U64, b"max"), (b"s-edge", 1, b"1"), (b"t-edge", H, b"h"), (b"t-edge", 0, b"0")]
    r2 = [(b"s-edge", H - 1, b"h-1"), (b"t-edge", U64, b"max"), (b"t-edge", 1, b"1")]
    return cc.case_of_runs([r0, r1, r2], wm=H)


def check_u64_edges(case):
    ents = [case.kv.entry(int(i)) for i in newest_order(case)]
    want = [U64, 1 << 63, (1 << 63) - 1, 1, 0]
    assert [ts for k, ts, _ in ents if k == b"s-edge"] == want == [ts for k, ts, _ in ents if k == b"t-edge"]
    signed = lambda t: t - (1 << 64) if t >> 63 else t
    assert sorted(want, key=signed, reverse=True) != want


# ------------------------------------------------------------------------------ key ties
KEY_TIES = ("tails", "prefix16", "zero_pad")


def key_ties():
    """Pairs of keys (A < B) whose zero-padded 16-byte images tie, A's versions in runs 0 and 1 and
    B's in runs 1 and 2 with interleaved ts, so a search for an A entry in run 1 ties on the image
    against both keys, goes through key_cmp in global memory and then to the ts:
      tails     both keys over 16 bytes, differing in the tail
      prefix16  A exactly 16 bytes and a prefix of B
      zero_pad  A shorter than 16 bytes, B = A zero-extended to 16 bytes"""
    P = b"sixteen-byte-key"
    assert len(P) == 16
    pairs = dict(tails=(b"T" * 16 + b"tail-a", b"T" * 16 + b"tail-b"), prefix16=(P, P + b"\0x"),
                 zero_pad=(b"pad", b"pad" + b"\0" * 13))
    runs = [[], [], []]
    for name in sorted(pairs, key=lambda n: pairs[n][0]):
        A, B = pairs[name]
        runs[0] += [(A, 9, b"a0.9"), (A, 6, b""), (A, 3, b"a0.3")]
        runs[1] += [(A, 8, b"a1.8"), (A, 6, b"a1.6"), (A, 2, b"a1.2"), (B, 7, b"b1.7"), (B, 4, b"b1.4")]
        runs[2] += [(B, 9, b"b2.9"), (B, 5, b""), (B, 4, b"b2.4"), (B, 1, b"b2.1")]
    return cc.case_of_runs(runs, pairs=pairs)


def check_key_ties(case):
    img = lambda k: k[:16].ljust(16, b"\0")
    pairs = case.info["pairs"]
    assert set(pairs) == set(KEY_TIES)
    for A, B in pairs.values():
        assert A < B and img(A) == img(B)
    A, B = pairs["tails"]
    assert len(A) > 16 and len(B) > 16 and A[:16] == B[:16]
    A, B = pairs["prefix16"]
    assert len(A) == 16 and B.startswith(A)
    A, B = pairs["zero_pad"]
    assert len(A) < 16 and len(B) == 16 and B == A.ljust(16, b"\0")
    multi = multi_run_keys(case)
    assert all(A in multi and B in multi for A, B in pairs.values())
    return len(multi)


# ------------------------------------------------------------------------------ tile limits
TILE_KERNELS = ("tile", "tile", "big", "big", "global")


def tile_limit_sizes(c=C):
    return (c.kMTE - 1, c.kMTE, c.kMTE + 1, c.kBigTE, c.kBigTE + 1)


def _tile_limit_runs(hot):
    H = b"hot-key-%d" % hot
    runs = [[(b"a-low-%d" % r, 5 + r, b"lo")] for r in range(3)]
    for j in range(hot):   # version j (ts descending) in run j % 3: the merged order takes the runs in turn
        runs[j % 3].append((H, 3 * hot - j, b"%d" % j if j % 5 else b""))
    for r in range(3):
        runs[r] += [(b"z-high-%d" % i, 9, b"hi") for i in (r, r + 3)]
    return runs, H


def tile_limit(X, c=C):
    """A hot key whose tile holds exactly X entries -- its versions spread round-robin over three
    runs, then the filler keys up to the next candidate -- with filler keys on both sides."""
    for hot in range(X, max(X - 16, 2), -1):
        runs, H = _tile_limit_runs(hot)
        case = cc.case_of_runs(runs, X=X, hot=H)
        if cc.tile_totals(case.kv, case.rs, c).max() == X:
            return case
    raise AssertionError(f"no tile of {X} entries")


def check_tile_limit(case, c=C):
    """The case's largest tile holds the X entries it was built for, X is one of the limits of
    `c`, and every other tile is filler; -> the kernel that merges it."""
    X = case.info["X"]
    assert X in tile_limit_sizes(c), (X, tile_limit_sizes(c))
    total = np.sort(cc.tile_totals(case.kv, case.rs, c))
    assert total[-1] == X and (total[:-1] <= 3).all(), total[-4:]
    assert case.info["hot"] in multi_run_keys(case)
    return cc.tile_kernel(int(total[-1]), c)


# ------------------------------------------------------------------------------ run counts
def many_runs(seed=3):
    """64 runs of 1 to 3 entries over 12 keys: every key in many runs, equal ts among them."""
    rng = np.random.default_rng(seed)
    runs = []
    for r in range(64):
        picks = sorted({(int(rng.integers(0, 12)), int(rng.integers(1, 9))) for _ in range(int(rng.integers(1, 4)))},
                       key=lambda p: (p[0], -p[1]))
        runs.append([(b"key-%02d" % k, ts, b"" if (r + ts) % 6 == 0 else b"%d.%d" % (r, ts)) for k, ts in picks])
    return cc.case_of_runs(runs)


def empty_runs():
    """Empty runs at the front, in the middle and at the end."""
    a = [(b"k", 9, b"a9"), (b"k", 4, b"a4"), (b"p", 2, b"")]
    b = [(b"j", 1, b"b1"), (b"k", 6, b"b6"), (b"k", 4, b"b4")]
    return cc.case_of_runs([[], a, [], [], b, []])


def single_run():
    """nrun == 1: the merge is the identity."""
    return cc.case_of_runs([[(b"a", 3, b"x"), (b"a", 1, b""), (b"b", 7, b"y"), (b"c" * 40, 2, b"z")]])


def no_entries():
    return cc.case_of_runs([[], []])


def disjoint_runs(seed=4):
    """No key lives in two runs: the NEWEST order is MergeIterator's."""
    rng = np.random.default_rng(seed)
    runs = [[] for _ in range(4)]
    for i in range(300):
        r = int(rng.integers(0, 4))
        for ts in sorted(rng.choice(50, int(rng.integers(1, 4)), replace=False).tolist(), reverse=True):
            runs[r].append((b"d%04d" % i, ts + 1, b"v%d" % ts))
    return cc.case_of_runs(runs)


# ------------------------------------------------------------------------------ candidate edges
def cand_edge_lengths(c=C):
    return (c.kMS - 1, c.kMS, c.kMS + 1, 2 * c.kMS + 1)


def cand_edges(c=C):
    """Runs of kMS - 1, kMS, kMS + 1 and 2 kMS + 1 entries that share the key S: the last entry of
    the first two, entry kMS (a candidate) of the third, and entries kMS .. 2 kMS of the fourth (its
    candidates kMS and 2 kMS), ts interleaved over the runs."""
    S = b"m-shared"
    low = lambda r, i: (b"c%05d" % (4 * i + r), 5, b"v%d" % (i % 7))
    runs = []
    for r, ln in enumerate(cand_edge_lengths(c)):
        nlow = min(ln - 1, c.kMS)
        run = [low(r, i) for i in range(nlow)]
        run += [(S, 4000 - 4 * j - r, b"" if j % 9 == 4 else b"s%d.%d" % (r, j)) for j in range(ln - nlow)]
        runs.append(run)
    return cc.case_of_runs(runs, S=S)


def check_cand_edges(case, c=C):
    rs = case.rs.astype(np.int64)
    assert tuple(np.diff(rs).tolist()) == cand_edge_lengths(c), (np.diff(rs), cand_edge_lengths(c))
    S = case.info["S"]
    for r in (2, 3):
        assert case.kv.entry(int(rs[r]) + c.kMS)[0] == S and case.kv.entry(int(rs[r]) + c.kMS - 1)[0] != S
    assert case.kv.entry(int(rs[3]) + 2 * c.kMS)[0] == S
    assert case.kv.entry(int(rs[1]) - 1)[0] == S and case.kv.entry(int(rs[2]) - 1)[0] == S
    return int(cc.tile_totals(case.kv, case.rs, c).max())


# ------------------------------------------------------------------------------ rules
def rules_cases():
    """[(name, case, watermark, bottom_level, prefixes, block_size, target_sst_size)] over
    interleaved(), equal_ts(), u64_edges() and key_ties(): a watermark between two runs' versions of
    one key (k-inter at 6: the survivor at or below it is run 1's, the newest version run 0's), a
    tombstone that is the overall newest version in a non-first run with bottom_level (t-tomb, and
    u-tomb whose tombstone is run 0's newest only), prefix filters, the ts edges as watermarks."""
    it, eq, u, kt = interleaved(), equal_ts(), u64_edges(), key_ties()
    out = []
    for wm in (0, 4, 6, 8, 9):
        for bottom in (False, True):
            out.append((f"inter-wm{wm}-b{int(bottom)}", it, wm, bottom, (), 4096, 1 << 20))
    out.append(("inter-prefix", it, 6, True, (b"k-", b"u"), 64, 1))
    out.append(("inter-prefix-all", it, 9, False, (b"",), 4096, 1 << 20))
    for wm in (3, 4, U64):
        out.append((f"equal-wm{wm}", eq, wm, wm == 4, (), 64, 100))
    for wm in (0, 1, (1 << 63) - 1, 1 << 63, U64):
        out.append((f"u64-wm{wm}", u, wm, wm == 1, (), 4096, 1 << 20))
    out.append(("ties-wm5", kt, 5, True, (b"pad\0",), 128, 200))
    out.append(("ties-wm6", kt, 6, False, (), 64, 1))
    return out


def check_rules_cases(cases):
    """The rule classes the cases reach (asserted: all of them)."""
    seen = set()
    for name, case, wm, bottom, pf, bs, target in cases:
        src = newest_order(case)
        ents = [case.kv.entry(int(i)) for i in src]
        run = run_of(case, src)
        kept = set(O.compact(case.kv, src, wm, bottom, pf, bs, target, kept_only=True)["kept"].tolist())
        by_key = {}
        for j, (k, ts, v) in enumerate(ents):
            by_key.setdefault(k, []).append((j, ts, v, int(run[j])))
        for k, vs in by_key.items():
            runs = {x[3] for x in vs}
            below = [x for x in vs if x[1] <= wm]
            if len(runs) < 2:
                continue
            if below and len(below) < len(vs) and below[0][3] != vs[-len(below) - 1][3]:
                seen.add("watermark_between_runs")
            if below and below[0][0] in kept and below[0][3] > vs[0][3]:
                seen.add("survivor_from_higher_run")
            if bottom and not vs[0][2] and vs[0][1] <= wm and vs[0][3] > min(runs) and not any(x[0] in kept for x in vs):
                seen.add("newest_tombstone_in_later_run_dropped")
            if bottom and any(not x[2] and x[3] == min(runs) for x in vs) and vs[0][2] and vs[0][0] in kept:
                seen.add("first_run_tombstone_not_newest")
            if pf and any(k.startswith(p) for p in pf) and below and below[0][0] not in kept:
                seen.add("prefix_filtered")
            if len({x[1] for x in below}) < len(below) and below[0][0] in kept:
                seen.add("equal_ts_survivor_is_lower_run")
    want = {"watermark_between_runs", "survivor_from_higher_run", "newest_tombstone_in_later_run_dropped",
            "first_run_tombstone_not_newest", "prefix_filtered", "equal_ts_survivor_is_lower_run"}
    assert want <= seen, sorted(want - seen)
    return seen


# ------------------------------------------------------------------------------ rotation
ROT_BS, ROT_TARGET = 128, 300


def rotation(nkeys=120):
    """Keys of three versions, one in each of three runs with the runs' turn changing from key to
    key, ~20-byte values: at block_size 128 and target_sst_size 300 an SST reaches its target
    every few entries, often inside a key's versions, where same_as_last_key holds the cut back."""
    runs = [[], [], []]
    for i in range(nkeys):
        key = b"rot-%04d" % i
        for j in range(3):
            runs[(i + j) % 3].append((key, 90 - 10 * j - i % 7, b"value-%04d-%d-" % (i, j) + b"x" * (i % 9)))
    return cc.case_of_runs(runs)


def check_rotation(case, bs=ROT_BS, target=ROT_TARGET):
    """SSTs whose cut was held back over versions of one key that come from different runs: the
    SST's finished blocks reach the target at entry p (the first entry checked after the block that
    reaches it was finished), the cut falls at e > p, and [p - 1, e) is one key from several runs."""
    src, want = expected_compact(case, 0, False, (), bs, target)
    kept = src[want["kept"]]
    ents = [case.kv.entry(int(i)) for i in kept]
    run = run_of(case, kept)
    cnt = pc.block_entry_counts(want["blocks"], want["blk_off"].astype(np.int64))
    first = np.concatenate([[0], np.cumsum(cnt)])          # every block's first kept entry
    size = np.diff(want["blk_off"].astype(np.int64)) + 4   # block + CRC
    held = 0
    for s in range(len(want["sst_blk"]) - 2):
        b0, b1, e = int(want["sst_blk"][s]), int(want["sst_blk"][s + 1]), int(want["sst_ent"][s + 1])
        cum = np.cumsum(size[b0:b1])
        j = int(np.searchsorted(cum, target, "left")) + 1   # blocks b0 .. b0 + j - 1 finished: >= target
        if b0 + j >= b1:
            continue
        p = int(first[b0 + j]) + 1                          # block b0 + j - 1 is finished by the add of first[b0 + j]
        if e > p:
            assert len({ents[x][0] for x in range(p - 1, e)}) == 1
            held += len({int(run[x]) for x in range(p - 1, e)}) > 1
        assert ents[e][0] != ents[e - 1][0]
    assert held >= 3 and len(want["sst_ent"]) > 20, (held, len(want["sst_ent"]))
    return held, len(want["sst_ent"]) - 1


# ------------------------------------------------------------------------------ all merge cases
def merge_cases():
    """{name: case} for the merge parity: every generator above."""
    out = dict(interleaved=interleaved(), equal_ts=equal_ts(), u64_edges=u64_edges(), key_ties=key_ties(),
               many_runs=many_runs(), empty_runs=empty_runs(), single_run=single_run(), no_entries=no_entries(),
               disjoint=disjoint_runs(), cand_edges=cand_edges(), rotation=rotation())
    for X in tile_limit_sizes():
        out[f"tile_{X}"] = tile_limit(X)
    return out
