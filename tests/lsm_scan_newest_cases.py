"""Snapshot range scans over an LSM view (LSMBLK_LSM_SCAN_NEWEST) -- TEST INFRASTRUCTURE.

The method of lsm_scan_cases.py for the scan's third mode, the (key ascending, ts descending) merge of
every source; shared by test_lsm_scan_newest_cases.py (CPU: three independent routes to every
expectation, and the generators reach what they were built for) and test_gpu_lsm_scan_newest.py
(GPU: every result field, seg_start, the stats and every byte of both streams).

  views         every case of lsm_scan_cases, and `versions`, built for the ts-aware rank
  closed form   closed_newest(): lsm_scan_cases.runs_of with the corrected landing, a stable sort of
                every run entry by (key, -ts, source ordinal, position), scan_cases.read_filter_rule
                (nothing when read_ts is None)
  plain         plain_newest(): per key a maximum over every version of every table within the
                bounds -- no runs, no merge, no predecessor rule
  line by line  line_by_line_newest(): the iterators lsm_scan_cases builds for scan_with_ts under a
                heap merge on (key, Reverse(ts), index) that never skips an equal key, read through
                lsm_scan_cases.BoundedLsmIterator
"""
import heapq
from functools import lru_cache

import get_cases as gc
import lsm_get_cases as lc
import lsm_scan_cases as ls
import scan_cases as sc

UNBOUNDED, INCLUDED, EXCLUDED = ls.UNBOUNDED, ls.INCLUDED, ls.EXCLUDED
OK, EMPTY = ls.OK, ls.EMPTY
FIELDS = ls.FIELDS
NEWEST = 4  # LSMBLK_LSM_SCAN_NEWEST
MODES = ("view", "merged")  # with q_ts, and q_ts = NULL
TS_MAX, TS_MID, RUN_LENGTHS, T = ls.TS_MAX, ls.TS_MID, ls.RUN_LENGTHS, ls.T


# ------------------------------------------------------------------------------ (a) the closed form
def closed_newest(v, lk, lo, uk, up, read_ts):
    """One range -> the result record's fields, its runs and its output entries."""
    runs = ls.runs_of(v, lk, lo, uk, up, mvcc=True)
    if runs is None:
        return dict(status=EMPTY, sources=0, raw=0, merged=0, n=0, runs=[], out=[])
    tagged = [(e[0], -e[1], src, pos, e) for src, (_, run) in enumerate(runs) for pos, e in enumerate(run)]
    merged = [x[4] for x in sorted(tagged, key=lambda x: x[:4])]
    out = merged if read_ts is None else sc.read_filter_rule(merged, read_ts)
    raw = sum(len(r) for _, r in runs)
    return dict(status=OK if out else EMPTY, sources=len(runs), raw=raw, merged=raw, n=len(out), runs=[r for _, r in runs],
                out=out)


# ------------------------------------------------------------------------------ (b) a plain maximum
def in_bounds(key, lk, lo, uk, up):
    if (lk == INCLUDED and key < lo) or (lk == EXCLUDED and key <= lo):
        return False
    return ls.within(key, uk, up)


def plain_newest(v, lk, lo, uk, up, read_ts):
    """Per key of any table that lies within the bounds: the version that is greatest by
    (ts <= read_ts, ts, -source ordinal) over every table, emitted iff it is visible and its value is
    not empty; keys ascending."""
    if (lk and not lo) or (uk and not up):
        return []
    best = {}
    for src, t in enumerate(ls.tables(v)):
        for k, ts, val in lc.flat(v.ssts[t])[0]:
            if in_bounds(k, lk, lo, uk, up):
                rank = (ts <= read_ts, ts, -src)
                if k not in best or rank > best[k][0]:
                    best[k] = (rank, (k, ts, val))
    return [e for k, (rank, e) in sorted(best.items()) if rank[0] and e[2]]


def every_version(v, lk, lo, uk, up):
    """The multiset the merged stream must hold: every entry of every table within the bounds."""
    if (lk and not lo) or (uk and not up):
        return []
    return sorted(e for t in ls.tables(v) for e in lc.flat(v.ssts[t])[0] if in_bounds(e[0], lk, lo, uk, up))


# ------------------------------------------------------------------------------ (c) line by line
class SnapshotMergeIterator:
    """A heap merge of StorageIterators on (key, Reverse(ts), index): every entry of every iterator,
    keys ascending, a key's versions newest first, the lower index first at an equal ts.  Unlike
    MergeIterator (src/iterators/merge_iterator.rs:130-169) next() never advances another iterator
    past an equal key."""

    def __init__(self, iters):
        self.iters, self.heap = iters, []
        for idx, it in enumerate(iters):
            self._push(idx)

    def _push(self, idx):
        it = self.iters[idx]
        if it.is_valid():
            k, ts, _ = it.entry()
            heapq.heappush(self.heap, (k, -ts, idx))

    def is_valid(self):
        return bool(self.heap)

    def entry(self):
        return self.iters[self.heap[0][2]].entry()

    def next(self):
        idx = heapq.heappop(self.heap)[2]
        self.iters[idx].next()
        self._push(idx)


def source_iterators(v, lk, lo, uk, up):
    """scan_with_ts's iterators with the corrected landing (lsm_scan_cases.merge_iterator's list)."""
    iters = [ls.table_iter(v.ssts[t], lk, lo, True) for t in v.l0 if ls.passes(v.ssts[t], lk, lo, uk, up)]
    for lv in v.levels:
        iters.append(ls.level_iter([v.ssts[t] for t in lv if ls.passes(v.ssts[t], lk, lo, uk, up)], lk, lo, True))
    return iters


def line_by_line_newest(v, lk, lo, uk, up, read_ts):
    if (lk and not lo) or (uk and not up):
        return []
    inner = SnapshotMergeIterator(source_iterators(v, lk, lo, uk, up))
    out = []
    if read_ts is None:
        while inner.is_valid() and ls.within(inner.entry()[0], uk, up):
            out.append(inner.entry())
            inner.next()
        return out
    it = ls.BoundedLsmIterator(inner, (uk, up), read_ts)
    while it.is_valid():
        out.append(it.entry())
        it.next()
    return out


# ------------------------------------------------------------------------------ cases
MANY = 70  # versions of m-many in one table
SPECIAL = (b"e-equal", b"h-high", b"m-many", b"t-tomb", b"x-inter")


def _versions(bs):
    """A view built for the ts-aware rank; every key starts with the 20-byte TIE_PREFIX, so every
    image compare ties and the full-key and ts compares decide.  L0 a, L0 b, level 0 = {c1}, level 1 = {c2}.
      x-inter   ts interleaved over three sources: a {900, 300}, b {700, 500}, c2 {800, 100}
      e-equal   ts 400 in a, b and c2, each with its own value
      t-tomb    c2's tombstone at 450 over a's older value at 200
      h-high    a holds only versions above TS_MID, b and c2 visible ones
      m-many    MANY versions in c2 (ts 990, 980 .. 300, every seventh a tombstone) over several
                blocks, interleaved with a's two (655, 345)
      r0000 ..  130 single-version keys in c1 (ranges of 0, 1, 63, 64, 65, 130 entries of it), every
                third also in a with a newer ts, every fifth also in b with an older one"""
    k = lambda x: T + x
    r = lambda i: k(b"r%04d" % i)
    a = [(r(i), 700 + i % 5, b"new%d" % i if i % 9 else b"") for i in range(0, 130, 3)]
    a += [(k(b"x-inter"), 900, b"a900"), (k(b"x-inter"), 300, b"a300"), (k(b"e-equal"), 400, b"ea"), (k(b"t-tomb"), 200, b"a200"),
          (k(b"h-high"), 900, b"a900"), (k(b"h-high"), 800, b""), (k(b"m-many"), 655, b"a655"), (k(b"m-many"), 345, b"a345")]
    b = [(r(i), 50, b"older%d" % i) for i in range(0, 130, 5)]
    b += [(k(b"x-inter"), 700, b"b700"), (k(b"x-inter"), 500, b""), (k(b"e-equal"), 400, b"eb"), (k(b"h-high"), 300, b"b300")]
    c1 = [(r(i), 100, b"old%d" % i) for i in range(130)]
    c2 = [(k(b"x-inter"), 800, b"c800"), (k(b"x-inter"), 100, b"c100"), (k(b"e-equal"), 400, b"ec"), (k(b"t-tomb"), 450, b""),
          (k(b"h-high"), 250, b"c250")]
    c2 += [(k(b"m-many"), 990 - 10 * i, b"m%d" % i if i % 7 else b"") for i in range(MANY)]
    ents = [sorted(x, key=lambda e: (e[0], -e[1])) for x in (a, b, c1, c2)]
    ssts = [gc.make_sst(e, bs) for e in ents]
    v = lc.View("versions", ssts, [0, 1], [[2], [3]], [], [])
    c = ls.Case("versions", bs, v, [], [], [], [], [])
    for n in RUN_LENGTHS:  # exactly n entries of the level table c1
        if n == 0:
            c.add(INCLUDED, r(1) + b"a", INCLUDED, r(1) + b"b")
        else:
            c.add(INCLUDED, r(0), INCLUDED, r(n - 1))
            if n + 1 < 130:
                c.add(EXCLUDED, r(0), EXCLUDED, r(n + 1))
    for key in SPECIAL:  # point ranges at every version's ts and just below it
        tss = sorted({ts for e in ents for kk, ts, _ in e if kk == k(key)})
        c.add(INCLUDED, k(key), INCLUDED, k(key), tuple(x for ts in tss for x in (ts - 1, ts)) + (TS_MAX,))
    for i in (0, 3, 5, 15, 7):  # r keys in a and b, in a, in b, in both, in c1 alone
        c.add(INCLUDED, r(i), INCLUDED, r(i), (49, 50, 99, 100, 699, 705, TS_MAX))
    c.add(UNBOUNDED, b"", UNBOUNDED, b"")
    c.add(INCLUDED, k(b"e"), EXCLUDED, k(b"zz"))
    c.add(EXCLUDED, k(b"m-many"), INCLUDED, k(b"x-inter"))
    c.add(INCLUDED, k(b"h-high"), EXCLUDED, k(b"m-many"))
    c.add(INCLUDED, T[:gc.IMG_BYTES], INCLUDED, T + b"\xff")
    ls.gen_ranges(c, 78, 3, 40)
    return c


CASES = ls.CASES + (("versions", 128),)


@lru_cache(maxsize=None)
def case(name, bs):
    return _versions(bs) if name == "versions" else ls.case(name, bs)


@lru_cache(maxsize=None)
def rows(name, bs, mode):
    c = case(name, bs)
    return [closed_newest(c.view, lk, lo, uk, up, ts if mode == "view" else None) for lk, lo, uk, up, ts in c.ranges()]


@lru_cache(maxsize=None)
def expected(name, bs, mode):
    return ls.arrays(rows(name, bs, mode))


def point_ranges(name, bs):
    """Indices of the case's ranges [Included(k), Included(k)]."""
    c = case(name, bs)
    return [i for i, (lk, lo, uk, up, _) in enumerate(c.ranges()) if lk == uk == INCLUDED and lo == up]


def disjoint(runs):
    """No key lives in two runs."""
    seen = set()
    for _, run in runs:
        keys = {e[0] for e in run}
        if keys & seen:
            return False
        seen |= keys
    return True


# ------------------------------------------------------------------------------ coverage classifiers
CLASSES = ("interleaved_ts_3_sources", "equal_ts_two_sources", "winner_not_highest_priority", "lower_priority_tombstone_hides",
           "same_key_stretch_ge_65", "over_64_runs", "newest_differs_from_mvcc", "all_image_tie") + \
    tuple("run_len_%d" % n for n in RUN_LENGTHS)


@lru_cache(maxsize=None)
def classes(name, bs):
    """Counts of the input classes the case reaches (ranges; newest_differs_from_mvcc: rows)."""
    c, v = case(name, bs), case(name, bs).view
    n = dict.fromkeys(CLASSES, 0)
    for lk, lo, uk, up, ts in c.ranges():
        runs = ls.runs_of(v, lk, lo, uk, up, True)
        if runs is None:
            continue
        n["over_64_runs"] += len(runs) > 64
        for x in RUN_LENGTHS:
            n["run_len_%d" % x] += any(len(e) == x for _, e in runs)
        new, old = closed_newest(v, lk, lo, uk, up, ts)["out"], ls.closed(v, lk, lo, uk, up, True, ts)["out"]
        n["newest_differs_from_mvcc"] += len(set(new) ^ set(old)) if new != old else 0
        raw = [e for _, ents in runs for e in ents]
        n["all_image_tie"] += sum(1 for _, e in runs if e) >= 2 and len({e[0] for e in raw}) >= 2 and \
            len({gc.image(e[0]) for e in raw}) == 1
        holders = {}
        for src, (_, ents) in enumerate(runs):
            for pos, (key, ets, val) in enumerate(ents):
                holders.setdefault(key, []).append((-ets, src, pos, val))
        hit = dict.fromkeys(CLASSES[:5], False)
        for key, h in holders.items():
            srcs = sorted({x[1] for x in h})
            if len(srcs) < 2:
                continue
            order = [x[1] for x in sorted(h)]  # the sources of the key's versions in merged order
            hit["interleaved_ts_3_sources"] |= len(srcs) >= 3 and order != sorted(order)
            tss = {}
            for nts, src, _, _ in h:
                tss.setdefault(nts, set()).add(src)
            hit["equal_ts_two_sources"] |= any(len(s) >= 2 for s in tss.values())
            hit["same_key_stretch_ge_65"] |= any(sum(1 for x in h if x[1] == s) >= 65 for s in srcs)
            seen = [x for x in sorted(h) if -x[0] <= ts]
            if seen:
                win = seen[0]
                hit["winner_not_highest_priority"] |= win[1] != srcs[0]
                hit["lower_priority_tombstone_hides"] |= win[1] != srcs[0] and not win[3] and \
                    any(x[1] < win[1] and x[3] for x in seen[1:])
        for key_, x in hit.items():
            n[key_] += x
    return {key_: int(x) for key_, x in n.items()}
