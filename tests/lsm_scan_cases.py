"""LSM views and range scans that reach chosen paths of lsmblk_lsm_scan_batch -- TEST INFRASTRUCTURE.

The method of lsm_get_cases.py / scan_cases.py for the range read over a whole view; shared by
test_lsm_scan_cases.py (CPU: two independent routes to every expectation, and the generators reach
what they were built for) and test_gpu_lsm_scan.py (GPU: every result field, seg_start, the stats
and every byte of both streams against the expectation).

  views         lsm_get_cases' mixed / levels / ties / threshold, and `owners`, built for the merge
  closed form   closed(): per passing table scan_cases.scan_one, pyref.merge_runs_rule over the runs
                in priority order, scan_cases.read_filter_rule (nothing when read_ts is None)
  line by line  line_by_line(): the iterators scan_with_ts builds (src/lsm_storage.rs:474-538) --
                per L0 table range_overlap, the table seek and the Excluded skip; per level the
                filtered table list, SstConcatIterator's seek and the Excluded skip --
                pyref.MergeIterator over them in source order, and BoundedLsmIterator, which is
                scan_cases.LsmIterator with the end bound tested on the first position as well
"""
import bisect
from dataclasses import dataclass
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import get_cases as gc
import lsm_get_cases as lc
import scan_cases as sc
from oracle import pyref

UNBOUNDED, INCLUDED, EXCLUDED = sc.UNBOUNDED, sc.INCLUDED, sc.EXCLUDED
OK, EMPTY = sc.OK, sc.EMPTY
FIELDS = ("status", "sources", "raw", "merged", "n")
MODES = ("default", "mvcc", "merged")  # the two landings with q_ts, and q_ts = NULL (default landing)
TS_MAX = (1 << 64) - 1
TS_MID = 500  # the generators draw timestamps from [1, 1000)
RUN_LENGTHS = (0, 1, 63, 64, 65, 130)  # the rank kernel's lane and tile edges
T = lc.TIE_PREFIX


# ------------------------------------------------------------------------------ (a) the closed form
def tables(v):
    """The view's tables in priority order."""
    return list(v.l0) + [t for lv in v.levels for t in lv]


def passes(s, lk, lo, uk, up):
    return sc.range_overlap(lk, lo, uk, up, lc.first_key(s), lc.last_key(s))


_runs = {}


def runs_of(v, lk, lo, uk, up, mvcc):
    """[(table, its raw scan's entries)] over the passing tables in priority order; None for a bad range."""
    key = (id(v), lk, lo, uk, up, mvcc)
    if key not in _runs:
        if (lk and not lo) or (uk and not up):
            _runs[key] = None
        else:
            _runs[key] = [(t, sc.scan_one(v.ssts[t], lk, lo, uk, up, False, mvcc)["entries"])
                          for t in tables(v) if passes(v.ssts[t], lk, lo, uk, up)]
    return _runs[key]


def closed(v, lk, lo, uk, up, mvcc, read_ts):
    """One range -> the result record's fields, its runs and its output entries."""
    runs = runs_of(v, lk, lo, uk, up, mvcc)
    if runs is None:
        return dict(status=EMPTY, sources=0, raw=0, merged=0, n=0, runs=[], out=[])
    merged = pyref.merge_runs_rule([r for _, r in runs])
    out = merged if read_ts is None else sc.read_filter_rule(merged, read_ts)
    return dict(status=OK if out else EMPTY, sources=len(runs), raw=sum(len(r) for _, r in runs), merged=len(merged),
                n=len(out), runs=[r for _, r in runs], out=out)


# ------------------------------------------------------------------------------ (b) line by line
class BoundedLsmIterator(sc.LsmIterator):
    """scan_cases.LsmIterator with the end bound tested on the first position too (the quirk of
    LsmIterator::new, src/lsm_iterator.rs:29-43, is not reproduced by the library)."""

    def __init__(self, inner, end_bound, read_ts):
        self.inner, self.end_bound, self.read_ts = inner, end_bound, read_ts
        self.valid = inner.is_valid()
        if self.valid:
            kind, key = end_bound
            if kind == INCLUDED:
                self.valid = inner.entry()[0] <= key
            elif kind == EXCLUDED:
                self.valid = inner.entry()[0] < key
        self.prev_key = b""
        self.move_to_key()


def _skip_equal(it, key):  # :492-494 / :530-532
    while it.is_valid() and it.key() == key:
        it.next()
    return it


def table_iter(s, lk, lo, mvcc):  # :482-498
    if lk == UNBOUNDED:
        return lc.Run([(lc.flat(s)[0], 0)])
    it = lc.Run([lc.table_seek(s, lo, mvcc)])
    return _skip_equal(it, lo) if lk == EXCLUDED else it


def level_iter(tabs, lk, lo, mvcc):  # :520-536
    if lk == UNBOUNDED:
        return lc.Run([(lc.flat(s)[0], 0) for s in tabs])
    it = lc.concat_seek(tabs, lo, mvcc)
    return _skip_equal(it, lo) if lk == EXCLUDED else it


def merge_iterator(v, lk, lo, uk, up, mvcc):
    iters = [table_iter(v.ssts[t], lk, lo, mvcc) for t in v.l0 if passes(v.ssts[t], lk, lo, uk, up)]
    for lv in v.levels:
        iters.append(level_iter([v.ssts[t] for t in lv if passes(v.ssts[t], lk, lo, uk, up)], lk, lo, mvcc))
    return pyref.MergeIterator(iters)


def within(key, uk, up):
    return uk == UNBOUNDED or (key <= up if uk == INCLUDED else key < up)


def line_by_line(v, lk, lo, uk, up, mvcc, read_ts, iterator=BoundedLsmIterator):
    """What scan_with_ts yields below the memtables; read_ts None: the merged stream up to the bound."""
    if (lk and not lo) or (uk and not up):
        return []
    inner = merge_iterator(v, lk, lo, uk, up, mvcc)
    out = []
    if read_ts is None:
        while inner.is_valid() and within(inner.entry()[0], uk, up):
            out.append(inner.entry())
            inner.next()
        return out
    it = iterator(inner, (uk, up), read_ts)
    while it.is_valid():
        out.append(it.entry())
        it.next()
    return out


# ------------------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    bs: int
    view: object
    lower: list
    upper: list
    lkind: list
    ukind: list
    read_ts: list

    def add(self, lk, lo, uk, up, read_ts=(0, TS_MID, TS_MAX)):
        for ts in read_ts:
            self.lkind.append(lk)
            self.lower.append(lo if lk else b"")
            self.ukind.append(uk)
            self.upper.append(up if uk else b"")
            self.read_ts.append(ts)

    def __len__(self):
        return len(self.lower)

    def ranges(self):
        return zip(self.lkind, self.lower, self.ukind, self.upper, self.read_ts)


def view_pool(v, rng):
    """scan_cases.bound_pool over every entry of the view: keys, keys cut and extended, below and above."""
    return sc.bound_pool(SimpleNamespace(entries=[e for s in v.ssts for e in s.entries]), rng)


def gen_ranges(c, seed, per_pair, reach):
    """All nine bound-kind pairs, every range short: both sides bounded -- ranges between pool keys a
    few keys apart, lower > upper, lower == upper on a present key; one side unbounded -- the other
    near that end of the view; bounds on tables' first and last keys; the whole view once."""
    rng = np.random.default_rng(seed)
    pool, keys = view_pool(c.view, rng)
    step = lambda: int(rng.integers(0, reach))
    for lk in (INCLUDED, EXCLUDED):
        for uk in (INCLUDED, EXCLUDED):
            for _ in range(per_pair):
                i = int(rng.integers(0, len(pool)))
                c.add(lk, pool[i], uk, pool[min(i + step(), len(pool) - 1)])
            i = int(rng.integers(1, len(pool)))
            c.add(lk, pool[i], uk, pool[int(rng.integers(0, i))])  # lower > upper
            k = keys[int(rng.integers(0, len(keys)))]
            c.add(lk, k, uk, k)  # one present key
    for kind in (INCLUDED, EXCLUDED):
        for _ in range(2):
            c.add(UNBOUNDED, b"", kind, pool[min(step(), len(pool) - 1)])
            c.add(kind, pool[max(len(pool) - 1 - step(), 0)], UNBOUNDED, b"")
    c.add(UNBOUNDED, b"", UNBOUNDED, b"", (TS_MID,))
    # bounds on tables' first and last keys
    tabs = [c.view.ssts[t] for t in tables(c.view)]
    for s in (tabs[0], tabs[len(tabs) // 2], tabs[-1]):
        fk, lk_ = lc.first_key(s), lc.last_key(s)
        i, j = bisect.bisect_left(pool, fk), bisect.bisect_left(pool, lk_)
        for kind in (INCLUDED, EXCLUDED):
            c.add(kind, pool[max(i - 3, 0)], kind, fk, (TS_MAX,))
            c.add(kind, lk_, kind, pool[min(j + 3, len(pool) - 1)], (TS_MID,))
            c.add(kind, fk, kind, pool[min(i + 3, len(pool) - 1)], (TS_MID,))
    c.add(INCLUDED, pool[-1], UNBOUNDED, b"")  # above every table: no source
    c.add(UNBOUNDED, b"", EXCLUDED, pool[0])   # below every table


def _owners(bs):
    """A view built for the merge; every key starts with the 20-byte TIE_PREFIX, so every image
    compare of the merge and of the expansion ties.
      x-three   versions in three sources
      y-blind   the owner holds only versions newer than TS_MID, the next source a visible one
      z-tomb    the owner's visible version is a tombstone over an older value further down
      r0000 ..  130 single-version keys in one level table (ranges of 0, 1, 63, 64, 65, 130 entries of
                it), every third also in an L0 table, so the runs' ranks interleave"""
    k = lambda x: T + x
    r = lambda i: k(b"r%04d" % i)
    a = [(r(i), 700 + i % 5, b"new%d" % i if i % 9 else b"") for i in range(0, 130, 3)]
    a += [(k(b"x-three"), 90, b"a90"), (k(b"x-three"), 80, b"a80"), (k(b"y-blind"), 900, b"a900"), (k(b"y-blind"), 800, b""),
          (k(b"z-tomb"), 400, b""), (k(b"z-tomb"), 950, b"a950")]
    b = [(k(b"q-only-b"), 10, b"b10"), (k(b"x-three"), 70, b"b70"), (k(b"y-blind"), 300, b"b300"), (k(b"z-tomb"), 200, b"b200")]
    c1 = [(r(i), 100, b"old%d" % i) for i in range(130)]
    c2 = [(k(b"w-level"), 5, b"c5"), (k(b"x-three"), 60, b"c60"), (k(b"x-three"), 50, b""), (k(b"z-tomb"), 100, b"c100")]
    d = [(k(b"s-deep"), 1, b"d1"), (k(b"x-three"), 40, b"d40")]
    ents = [sorted(x, key=lambda e: (e[0], -e[1])) for x in (a, b, c1, c2, d)]
    ssts = [gc.make_sst(e, bs) for e in ents]
    v = lc.View("owners", ssts, [0, 1], [[2, 3], [4]], [], [])
    c = Case("owners", bs, v, [], [], [], [], [])
    for n in RUN_LENGTHS:  # exactly n entries of the level table c1
        if n == 0:
            c.add(INCLUDED, r(1) + b"a", INCLUDED, r(1) + b"b")
        else:
            c.add(INCLUDED, r(0), INCLUDED, r(n - 1))
            if n + 1 < 130:
                c.add(EXCLUDED, r(0), EXCLUDED, r(n + 1))
    for key in (b"x-three", b"y-blind", b"z-tomb"):
        c.add(INCLUDED, k(key), INCLUDED, k(key))
        for ts in (39, 40, 55, 60, 75, 85, 95, 150, 250, 350, 450, 850, 925, 960):
            c.add(INCLUDED, k(key), INCLUDED, k(key), (ts,))
    c.add(UNBOUNDED, b"", UNBOUNDED, b"")
    c.add(INCLUDED, k(b"q"), EXCLUDED, k(b"zz"))
    c.add(INCLUDED, T[:gc.IMG_BYTES], INCLUDED, T + b"\xff")
    c.add(EXCLUDED, T, EXCLUDED, T[:gc.IMG_BYTES] + b"\x00")  # lower > upper, images tie
    gen_ranges(c, 77, 4, 40)
    return c


VIEWS = ("mixed", "levels", "ties", "threshold")
CASES = tuple((n, bs) for n in VIEWS for bs in (128, 256)) + (("owners", 128),)


@lru_cache(maxsize=None)
def case(name, bs):
    if name == "owners":
        return _owners(bs)
    v = lc.case(name, bs)
    c = Case(name, bs, v, [], [], [], [], [])
    if name == "levels":  # the 70-table level whole: more than 64 runs in one range
        lv = [v.ssts[t] for t in v.levels[5]]
        assert len(lv) == lc.KARY + 6
        c.add(INCLUDED, lc.first_key(lv[0]), INCLUDED, lc.last_key(lv[-1]), (TS_MID,))
        c.add(EXCLUDED, lc.first_key(lv[0]), EXCLUDED, lc.last_key(lv[-1]), (0,))
        c.add(INCLUDED, lc.first_key(lv[2]), EXCLUDED, lc.first_key(lv[68]))  # a span inside the level
    gen_ranges(c, {"mixed": 1, "levels": 2, "ties": 3, "threshold": 4}[name] * 1000 + bs,
               per_pair={"mixed": 4, "levels": 6, "ties": 5, "threshold": 5}[name],
               reach={"mixed": 10, "levels": 30, "ties": 12, "threshold": 12}[name])
    return c


def mode_args(mode):
    """-> (mvcc, whether the reader's view applies)"""
    return mode == "mvcc", mode != "merged"


@lru_cache(maxsize=None)
def rows(name, bs, mode):
    c = case(name, bs)
    mvcc, filt = mode_args(mode)
    return [closed(c.view, lk, lo, uk, up, mvcc, ts if filt else None) for lk, lo, uk, up, ts in c.ranges()]


def arrays(rws):
    """Closed-form rows -> ({field: numpy array}, per-range out entries, per-run raw entries)."""
    out = {f: np.array([r[f] for r in rws], np.uint64) for f in FIELDS}
    return out, [r["out"] for r in rws], [run for r in rws for run in r["runs"]]


@lru_cache(maxsize=None)
def expected(name, bs, mode):
    return arrays(rows(name, bs, mode))


def query_counts():
    return sc.query_counts()


# ------------------------------------------------------------------------------ coverage classifiers
CLASSES = ("key_in_3_sources", "owner_blind_later_sees", "owner_tombstone", "level_span_ge_65", "begin_mid_versions",
           "excl_skip_across_block", "no_source", "merge_nonempty_view_empty", "all_image_tie", "over_64_runs",
           "lower_gt_upper", "first_position_beyond_bound") + tuple("run_len_%d" % n for n in RUN_LENGTHS)


@lru_cache(maxsize=None)
def classes(name, bs):
    """Counts of the input classes the case reaches, over both landings."""
    c, v = case(name, bs), case(name, bs).view
    n = dict.fromkeys(CLASSES, 0)
    for mvcc in (False, True):
        for lk, lo, uk, up, ts in c.ranges():
            runs = runs_of(v, lk, lo, uk, up, mvcc)
            if runs is None:
                continue
            r = closed(v, lk, lo, uk, up, mvcc, ts)
            n["no_source"] += not runs
            n["over_64_runs"] += len(runs) > 64
            n["lower_gt_upper"] += bool(lk and uk and lo > up)
            n["merge_nonempty_view_empty"] += r["merged"] > 0 and r["n"] == 0
            for x in RUN_LENGTHS:
                n["run_len_%d" % x] += any(len(e) == x for _, e in runs)
            for lv in v.levels:
                n["level_span_ge_65"] += sum(passes(v.ssts[t], lk, lo, uk, up) for t in lv) >= 65
            holders = {}
            for i, (_, ents) in enumerate(runs):
                for key in {e[0] for e in ents}:
                    holders.setdefault(key, []).append(i)
            n["key_in_3_sources"] += any(len(h) >= 3 for h in holders.values())
            for key, h in holders.items():
                if len(h) < 2:
                    continue
                own = [e for e in runs[h[0]][1] if e[0] == key]
                later = [e for i in h[1:] for e in runs[i][1] if e[0] == key]
                seen = [e for e in own if e[1] <= ts]
                n["owner_blind_later_sees"] += not seen and any(e[1] <= ts and e[2] for e in later)
                n["owner_tombstone"] += bool(seen) and not seen[0][2] and any(e[1] < seen[0][1] and e[2] for e in later)
            raw = [e for _, ents in runs for e in ents]
            n["all_image_tie"] += sum(1 for _, e in runs if e) >= 2 and len({e[0] for e in raw}) >= 2 and \
                len({gc.image(e[0]) for e in raw}) == 1
            if lk:
                for t, ents in runs:
                    s = v.ssts[t]
                    land = gc.seek_to_key_inner(s, lo, mvcc)
                    if land[0] >= len(s.blocks) or s.blocks[land[0]][land[1]][0] != lo:
                        continue
                    if lk == INCLUDED and not mvcc and ents and land != gc.seek_to_key_inner(s, lo, True):
                        n["begin_mid_versions"] += 1
                    if lk == EXCLUDED and sc.begin(s, lk, lo, mvcc)[0] != land[0]:
                        n["excl_skip_across_block"] += 1
            inner = merge_iterator(v, lk, lo, uk, up, mvcc)
            n["first_position_beyond_bound"] += inner.is_valid() and not within(inner.entry()[0], uk, up)
    return {k: int(x) for k, x in n.items()}


# ------------------------------------------------------------------------------ degenerate inputs
def corrupt_block(s, victim):
    """Table s with entry 0's offset of block `victim` pointing past the block's data (the scan does
    not check CRCs: the block breaks the decode rules)."""
    buf = bytearray(s.buf)
    end = s.ends[victim] - 4
    n = len(s.blocks[victim])
    buf[end - 2 - 2 * n:end - 2 * n] = (0xFFF0).to_bytes(2, "big")
    return bytes(buf)
