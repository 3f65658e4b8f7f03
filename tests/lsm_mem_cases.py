"""LSM views with memtable runs, point reads and range scans over them -- TEST INFRASTRUCTURE.

The method of lsm_get_cases.py / lsm_scan_cases.py / lsm_scan_newest_cases.py for views whose first
sources are memtable runs (lsmblk_lsm_view.mem); shared by test_lsm_mem_cases.py (CPU: two independent
routes to every expectation, and the generators reach what they were built for) and
test_gpu_lsm_mem.py (GPU: every result field, the stats and every byte against the closed form).

  views         the existing cases' tables at their small block sizes (or no table at all) plus runs
  closed form   per run a bisect landing and a version walk (mem_lookup) or a bisect slice (mem_slice),
                then lsm_get_cases.closed / lsm_scan_cases.runs_of with the ordinals shifted by nmem, the
                decider rule / the NEWEST maximum, pyref.merge_runs_rule / the snapshot sort, and
                scan_cases.read_filter_rule
  line by line  pyref.ListIter over what MemTable::scan yields of each run (get_with_ts: the key's
                versions, src/lsm_storage.rs:369-380; scan_with_ts: the entries within both bounds,
                :460-471) first in the MergeIterator list, then the table iterators of the existing
                cases, then LsmIterator / BoundedLsmIterator.  NEWEST: a plain per-key maximum over
                every run and table, and lsm_scan_newest_cases' heap merge
"""
import bisect
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import get_cases as gc
import lsm_get_cases as lc
import lsm_scan_cases as ls
import lsm_scan_newest_cases as lsn
import scan_cases as sc
from oracle import pyref

NONE = lc.NONE
ABSENT, FOUND, TOMBSTONE = lc.ABSENT, lc.FOUND, lc.TOMBSTONE
UNBOUNDED, INCLUDED, EXCLUDED = sc.UNBOUNDED, sc.INCLUDED, sc.EXCLUDED
KINDS = (UNBOUNDED, INCLUDED, EXCLUDED)
OK, EMPTY = sc.OK, sc.EMPTY
GET_FIELDS, GET_MODES, GET_FLAGS = lc.FIELDS, lc.MODES, lc.FLAGS
SCAN_FIELDS = ls.FIELDS
SCAN_MODES = ("default", "mvcc", "merged", "newest", "newest_merged")  # (landing, q_ts or NULL) and the snapshot merge
TS_MAX, TS_MID = ls.TS_MAX, ls.TS_MID
TS_MEM = 2000  # the runs draw timestamps from [1, 2000): newer than every table version, and older
MAX_MEM = 64
RUN_LENGTHS = (0, 1, 2, 63, 64, 65, 200)


@dataclass
class MemCase:
    name: str
    bs: int
    view: object    # lsm_get_cases.View: the tables (none: a database that never flushed)
    runs: list      # per memtable run its entries (key, ts, value) in (key ascending, ts descending) order
    keys: list      # the point reads
    read_ts: list
    scan: object    # lsm_scan_cases.Case: the ranges

    @property
    def nmem(self):
        return len(self.runs)

    @property
    def start(self):
        return [0] + [int(x) for x in np.cumsum([len(r) for r in self.runs])]

    def stream(self):
        """The runs back to back: (key bytes, key_off, value bytes, val_off, ts, run_start)."""
        return sc.stream_of(self.runs)


def run_keys(run):
    return [e[0] for e in run]


# ------------------------------------------------------------------------------ (a) the closed forms
def mem_lookup(run, key, read_ts):
    """One run's point read -> (the landing is on the key, index of the visible version or None)."""
    i = bisect.bisect_left(run_keys(run), key)
    on = i < len(run) and run[i][0] == key
    while i < len(run) and run[i][0] == key:
        if run[i][1] <= read_ts:
            return on, i
        i += 1
    return on, None


def closed_get(c, key, read_ts, mode):
    """One key -> the result record's fields (a mem hit: val_pos relative to the run's values, "run"
    its ordinal) and the value."""
    out = dict(status=ABSENT, src=NONE, sst=NONE, hit_blk=NONE, hit_ent=NONE, vlen=0, ts=0, val_pos=None, value=None)
    seeks = 0
    if not key:
        return dict(out, seeks=0, bloom_out=0)
    for r, run in enumerate(c.runs):
        seeks += 1
        on, hit = mem_lookup(run, key, read_ts)
        pick = None
        if hit is not None:
            _, ts, val = run[hit]
            pick = dict(out, status=FOUND if val else TOMBSTONE, src=r, hit_ent=c.start[r] + hit, vlen=len(val), ts=ts,
                        val_pos=sum(len(e[2]) for e in run[:hit]), value=val or None)
        if mode != "newest":
            if on:  # the decider: nothing after it is consulted
                return dict(pick or dict(out, src=r), seeks=seeks, bloom_out=0)
        elif pick and (out["src"] == NONE or pick["ts"] > out["ts"]):
            out = pick
    t = lc.closed(c.view, key, read_ts, mode)
    if t["src"] != NONE and (mode != "newest" or out["src"] == NONE or t["ts"] > out["ts"]):
        out = dict(t, src=t["src"] + c.nmem)
    return dict(out, seeks=seeks + t["seeks"], bloom_out=t["bloom_out"])


def mem_passes(run, lk, lo, uk, up):
    """A run is a source of the range iff it is not empty and passes range_overlap on its first and last key."""
    return bool(run) and sc.range_overlap(lk, lo, uk, up, run[0][0], run[-1][0])


def mem_slice(run, lk, lo, uk, up):
    """[begin, end) of the run for the bounds."""
    keys = run_keys(run)
    b = 0 if lk == UNBOUNDED else (bisect.bisect_left if lk == INCLUDED else bisect.bisect_right)(keys, lo)
    e = len(run) if uk == UNBOUNDED else (bisect.bisect_right if uk == INCLUDED else bisect.bisect_left)(keys, up)
    return b, max(b, e)


def bad_range(lk, lo, uk, up):
    return bool((lk and not lo) or (uk and not up))


def runs_of(c, lk, lo, uk, up, mvcc):
    """The range's raw runs in source order: the passing memtable runs' slices, then the passing tables' scans."""
    if bad_range(lk, lo, uk, up):
        return None
    out = []
    for run in c.runs:
        if mem_passes(run, lk, lo, uk, up):
            b, e = mem_slice(run, lk, lo, uk, up)
            out.append(run[b:e])
    return out + [r for _, r in ls.runs_of(c.view, lk, lo, uk, up, mvcc)]


def closed_scan(c, lk, lo, uk, up, mode, read_ts):
    """One range -> the result record's fields, its runs and its output entries."""
    newest = mode.startswith("newest")
    runs = runs_of(c, lk, lo, uk, up, newest or mode == "mvcc")
    if runs is None:
        return dict(status=EMPTY, sources=0, raw=0, merged=0, n=0, runs=[], out=[])
    if newest:
        tagged = [(e[0], -e[1], src, pos, e) for src, run in enumerate(runs) for pos, e in enumerate(run)]
        merged = [x[4] for x in sorted(tagged, key=lambda x: x[:4])]
    else:
        merged = pyref.merge_runs_rule(runs)
    out = merged if mode.endswith("merged") else sc.read_filter_rule(merged, read_ts)
    return dict(status=OK if out else EMPTY, sources=len(runs), raw=sum(len(r) for r in runs), merged=len(merged), n=len(out),
                runs=runs, out=out)


# ------------------------------------------------------------------------------ (b) line by line
def get_line_by_line(c, key, read_ts, mvcc):
    """get_with_ts over the runs and the view -> (value, ts) or None."""
    v = c.view
    iters = [pyref.ListIter([e for e in run if e[0] == key]) for run in c.runs]  # MemTable::scan(key ..= key)
    iters += [lc.Run([lc.table_seek(v.ssts[t], key, mvcc)]) for t in v.l0 if lc.keep_table(v.ssts[t], key)]
    for lv in v.levels:
        iters.append(lc.concat_seek([v.ssts[t] for t in lv if lc.keep_table(v.ssts[t], key)], key, mvcc))
    it = sc.LsmIterator(pyref.MergeIterator(iters), (UNBOUNDED, b""), read_ts)
    if it.is_valid() and it.entry()[0] == key and it.entry()[2]:
        return it.entry()[2], it.entry()[1]
    return None


def get_newest_plain(c, key, read_ts):
    """(ts, source ordinal, value) of the newest version <= read_ts over every run and every table that
    passes keep_table (the lower ordinal wins an equal ts), or None."""
    best = None
    for r, run in enumerate(c.runs):
        for k, ts, val in run:
            if k == key and ts <= read_ts and (best is None or ts > best[0]):
                best = (ts, r, val)
    t = lc.newest_plain(c.view, key, read_ts)
    if t is not None and (best is None or t[0] > best[0]):
        best = (t[0], t[1] + c.nmem, t[2])
    return best


def mem_scan_iter(run, lk, lo, uk, up):
    """MemTable::scan(lower, upper): the entries whose key lies within both bounds."""
    return pyref.ListIter([e for e in run if lsn.in_bounds(e[0], lk, lo, uk, up)])


def scan_line_by_line(c, lk, lo, uk, up, mode, read_ts):
    """What scan_with_ts yields over the runs and the view."""
    if bad_range(lk, lo, uk, up):
        return []
    v = c.view
    mem = [mem_scan_iter(run, lk, lo, uk, up) for run in c.runs]
    if mode.startswith("newest"):
        inner = lsn.SnapshotMergeIterator(mem + lsn.source_iterators(v, lk, lo, uk, up))
    else:
        mvcc = mode == "mvcc"
        tabs = [ls.table_iter(v.ssts[t], lk, lo, mvcc) for t in v.l0 if ls.passes(v.ssts[t], lk, lo, uk, up)]
        for lv in v.levels:
            tabs.append(ls.level_iter([v.ssts[t] for t in lv if ls.passes(v.ssts[t], lk, lo, uk, up)], lk, lo, mvcc))
        inner = pyref.MergeIterator(mem + tabs)
    out = []
    if mode.endswith("merged"):
        while inner.is_valid() and ls.within(inner.entry()[0], uk, up):
            out.append(inner.entry())
            inner.next()
        return out
    it = ls.BoundedLsmIterator(inner, (uk, up), read_ts)
    while it.is_valid():
        out.append(it.entry())
        it.next()
    return out


# ------------------------------------------------------------------------------ generators
def mk_run(entries):
    return sorted(entries, key=lambda e: (e[0], -e[1]))


def _val(rng, tomb=0.2):
    return b"" if rng.random() < tomb else bytes(rng.integers(0, 256, int(rng.integers(1, 30)), dtype=np.uint8))


def fill(rng, taken, old, n, fresh):
    """n further keys for a run: about half of `old` (keys the tables hold), the others from fresh() --
    each with one version (what a flush yields), about every fifth with two or three."""
    out, keys = [], set()
    while len(keys) < n:
        k = old[int(rng.integers(len(old)))] if old and rng.random() < 0.5 else fresh()
        if k and k not in taken and k not in keys:
            keys.add(k)
    for k in sorted(keys):
        nv = int(rng.integers(2, 4)) if rng.random() < 0.2 else 1
        for ts in sorted({int(t) for t in rng.integers(1, TS_MEM, nv)}, reverse=True):
            out.append((k, ts, _val(rng)))
    return out


def _exact(rng, n, taken, old, fresh, base=()):
    """`base` and whole keys from fill() until the run has exactly n entries."""
    ents = list(base)
    while len(ents) < n:
        more = fill(rng, taken | {e[0] for e in ents}, old, 1, fresh)
        if len(ents) + len(more) <= n:
            ents += more
    return ents


def table_keys(v):
    return sorted({k for s in v.ssts for k, _, _ in s.entries})


def holders(v, key):
    return [t for t in ls.tables(v) if any(k == key for k, _, _ in v.ssts[t].entries)]


def visible_value(v, key):
    """(ts, value) of the key's newest version in the view's deciding table when that is a value, else None."""
    r = lc.closed(v, key, TS_MAX, "mvcc")
    return (r["ts"], r["value"]) if r["status"] == FOUND else None


def point_queries(c, rng, extra):
    """Every key of the runs at chosen timestamps, the keys cut and extended, keys around every run, a
    share of the view's own queries, and `extra` (key, read_ts) pairs."""
    keys, ts = [], []
    mem = sorted({k for run in c.runs for k, _, _ in run})
    for k in mem:
        for t in (0, int(rng.integers(1, TS_MEM)), TS_MAX):
            keys.append(k)
            ts.append(t)
    for k in mem[::3]:
        for q in (k[:-1], k + b"a", k + b"\x00"):
            if q:
                keys.append(q)
                ts.append((int(rng.integers(1, TS_MEM)), TS_MAX)[int(rng.integers(2))])
    for run in c.runs:
        if run:
            for q in (run[0][0][:-1] or b"\x00", b"\x00", run[-1][0] + b"\xff", b"\xff\xff"):
                keys.append(q)
                ts.append(TS_MAX)
    for k, t in list(zip(c.view.keys, c.view.read_ts))[::4]:
        if k:
            keys.append(k)
            ts.append(t)
    for k, t in extra:
        keys.append(k)
        ts.append(t)
    c.keys, c.read_ts = keys, ts


def gen_mem_ranges(c, rng, share):
    """Ranges built around the runs: every bound-kind pair over short stretches of the runs' keys (cut
    and extended), bounds equal to a multi-version key, every nonempty run whole / one key / nothing
    between two neighbours / failing range_overlap below and above, and every `share`-th range of the
    view's own scan case."""
    s = c.scan
    mem = sorted({k for run in c.runs for k, _, _ in run})
    pool = sorted(set(mem) | {k[:-1] for k in mem if len(k) > 1} | {k + b"a" for k in mem[::3]} | {b"\x01", b"\xff\xff"})
    multi = sorted({a[0] for run in c.runs for a, b in zip(run, run[1:]) if a[0] == b[0]})
    pick_ts = lambda: (int(rng.integers(1, TS_MEM)),)
    for lk in KINDS:
        for uk in KINDS:
            for _ in range(3):
                i = int(rng.integers(0, len(pool)))
                s.add(lk, pool[i], uk, pool[min(i + int(rng.integers(0, 7)), len(pool) - 1)], pick_ts())
            if lk and uk:
                i = int(rng.integers(1, len(pool)))
                s.add(lk, pool[i], uk, pool[int(rng.integers(0, i))], (TS_MAX,))  # lower > upper
            for k in multi[:2]:  # the Excluded skip over all the versions, the Included end after them
                s.add(lk, k, uk, k, (TS_MAX,))
                s.add(lk, k, UNBOUNDED, b"", pick_ts())
                s.add(UNBOUNDED, b"", uk, k, pick_ts())
    for run in [r for r in c.runs if r][:4]:
        keys = sorted(set(run_keys(run)))
        first, last = keys[0], keys[-1]
        s.add(INCLUDED, first, INCLUDED, last, (TS_MID, TS_MAX))      # the whole run
        s.add(EXCLUDED, first, EXCLUDED, last, (TS_MAX,))
        s.add(INCLUDED, first, INCLUDED, first, (0, TS_MAX))          # one key
        s.add(INCLUDED, last, INCLUDED, last, (TS_MAX,))
        s.add(EXCLUDED, last, UNBOUNDED, b"", (TS_MAX,))              # range_overlap fails: above the run
        s.add(INCLUDED, last + b"\x00", UNBOUNDED, b"", (TS_MAX,))
        s.add(UNBOUNDED, b"", EXCLUDED, first, (TS_MAX,))             # ... and below it
        s.add(UNBOUNDED, b"", INCLUDED, first[:-1] or b"\x00", (TS_MAX,))
        if len(keys) > 1:  # passes, selects nothing: strictly between two neighbours
            i = len(keys) // 2
            s.add(EXCLUDED, keys[i - 1], EXCLUDED, keys[i], (TS_MAX,))
            s.add(INCLUDED, keys[i - 1] + b"\x00", EXCLUDED, keys[i], (TS_MAX,))
    s.add(UNBOUNDED, b"", UNBOUNDED, b"", (TS_MID, 1500, TS_MAX))
    if share and c.view.ssts and c.view.name in ls.VIEWS:
        t = ls.case(c.view.name, c.bs)
        for lk, lo, uk, up, ts in list(t.ranges())[::share]:
            s.add(lk, lo, uk, up, (ts,))


def _new(c_name, bs, view, runs):
    return MemCase(c_name, bs, view, [mk_run(r) for r in runs], [], [], ls.Case(c_name, bs, view, [], [], [], [], []))


SPECIAL = ("k_two_tables", "k_blind", "k_tomb", "k_equal")


def special_keys(v):
    """Four distinct keys of the view's tables: one held by two tables, three whose deciding table shows a value."""
    keys = table_keys(v)
    two = next(k for k in keys if len(holders(v, k)) >= 2)
    rest = [k for k in keys if k != two and visible_value(v, k) and visible_value(v, k)[0] >= 2][:60:20]
    return (two, *rest)


def _mixed3(bs):
    """lsm_get_cases' mixed view under three runs of 200, 64 and 63 entries.
      k_two_tables  in the mutable run, an immutable run and two tables
      k_blind       the mutable run holds only a version newer than the read, a table a visible one
      k_tomb        an immutable run's tombstone over a table's value
      k_equal       the ts of the table's visible version, in a run: NEWEST takes the run's
      m3            three versions in one run, read between them
      ab / abc      a prefix pair in one run, read on both sides of each"""
    rng = np.random.default_rng(31)
    v = lc.case("mixed", bs)
    two, blind, tomb, equal = special_keys(v)
    eq_ts, _ = visible_value(v, equal)
    r0 = [(two, 1500, b"mut-two"), (blind, TS_MEM, b"too-new"), (equal, eq_ts, b"mem-equal"), (b"ab", 1200, b"v-ab"),
          (b"abc", 1201, b"v-abc")]
    r1 = [(two, 1400, b"imm-two"), (tomb, 1600, b""), (b"m3", 30, b"m3-30"), (b"m3", 20, b""), (b"m3", 10, b"m3-10")]
    taken = {e[0] for e in r0 + r1}
    old = table_keys(v)
    fresh = lambda: old[int(rng.integers(len(old)))] + bytes([int(rng.integers(101, 110))])
    c = _new("mixed3", bs, v, [_exact(rng, n, taken, old, fresh, base) for base, n in ((r0, 200), (r1, 64), ([], 63))])
    extra = [(two, t) for t in (0, 900, 1450, 1550, TS_MAX)] + [(blind, TS_MEM - 1), (blind, TS_MEM), (tomb, TS_MAX), (tomb, 1599),
                                                                 (equal, eq_ts), (equal, eq_ts - 1), (equal, TS_MAX)]
    extra += [(b"m3", t) for t in (5, 10, 15, 20, 25, 30, 35)]
    extra += [(q, TS_MAX) for q in (b"a", b"ab", b"ab\x00", b"abb", b"abc", b"abca", b"abd")]
    point_queries(c, rng, extra)
    gen_mem_ranges(c, rng, 9)
    for k in (two, blind, tomb, equal, b"m3"):
        c.scan.add(INCLUDED, k, INCLUDED, k, (eq_ts, 1450, TS_MAX))
    return c


def _ties2(bs):
    """lsm_get_cases' ties view under runs of 65 and 1 entries whose keys share the 20-byte TIE_PREFIX:
    every image compare of a landing ties and the whole keys decide."""
    rng = np.random.default_rng(32)
    v = lc.case("ties", bs)
    old = table_keys(v)
    fresh = lambda: lc.TIE_PREFIX + bytes(rng.choice(list(b"abcd"), int(rng.integers(1, 7))).astype(np.uint8)) + b"m"
    r0 = _exact(rng, 65, set(), old, fresh)
    r1 = _exact(rng, 1, {e[0] for e in r0}, [], fresh)
    c = _new("ties2", bs, v, [r0, r1])
    extra = [(q, TS_MAX) for q in (lc.TIE_PREFIX, lc.TIE_PREFIX[:gc.IMG_BYTES], lc.TIE_PREFIX[:gc.IMG_BYTES] + b"\x00",
                                   lc.TIE_PREFIX + b"zzzz")]
    point_queries(c, rng, extra)
    gen_mem_ranges(c, rng, 11)
    return c


def _many67(bs):
    """The 72-source view (70 L0 tables, then levels of 64 and 65 tables) under runs of 2, 0 and 65
    entries: the table sources are ordinals 3 .. 74, so they cross the 64-lane batch edge, and a range
    over the whole key space has more than 64 runs."""
    rng = np.random.default_rng(33)
    v = lc.case("edges_72_sources", bs)
    old = table_keys(v)
    fresh = lambda: lc._num(int(rng.integers(0, 100 * (lc.KARY + 6))))
    r2 = _exact(rng, 65, set(), old, fresh)
    r0 = _exact(rng, 2, {e[0] for e in r2}, [], fresh)[:2]
    c = _new("many67", bs, v, [r0, [], r2])
    point_queries(c, rng, [])
    gen_mem_ranges(c, rng, 0)
    lv = [v.ssts[t] for t in v.l0]
    c.scan.add(INCLUDED, lc.first_key(lv[0]), INCLUDED, lc.last_key(lv[-1]), (TS_MID, TS_MAX))
    return c


def _nmem64(bs):
    """64 runs of 0, 1, 2, 3 and 5 entries over the levels view: every lane of the wave has a run."""
    rng = np.random.default_rng(34)
    v = lc.case("levels", bs)
    old = table_keys(v)
    fresh = lambda: lc._num(int(rng.integers(0, 100 * (lc.KARY + 6))))
    runs = [_exact(rng, (0, 1, 2, 3, 5)[r % 5], set(), old, fresh) for r in range(MAX_MEM)]
    c = _new("nmem64", bs, v, runs)
    both = sorted({k for r in runs[:32] for k, _, _ in r} & {k for r in runs[32:] for k, _, _ in r})
    point_queries(c, rng, [(k, TS_MAX) for k in both])
    gen_mem_ranges(c, rng, 13)
    return c


def _one(bs):
    rng = np.random.default_rng(35)
    v = lc.case("mixed", bs)
    old = table_keys(v)
    fresh = lambda: old[int(rng.integers(len(old)))] + bytes([int(rng.integers(101, 110))])
    c = _new("one", bs, v, [_exact(rng, 200, set(), old, fresh)])
    point_queries(c, rng, [])
    gen_mem_ranges(c, rng, 9)
    return c


def _allempty(bs):
    """Three runs without an entry: the view answers as it does without them, every ordinal shifted by three."""
    rng = np.random.default_rng(36)
    v = lc.case("mixed", bs)
    c = _new("allempty", bs, v, [[], [], []])
    point_queries(c, rng, [])
    c.keys, c.read_ts = c.keys[::2], c.read_ts[::2]
    t = ls.case("mixed", bs)
    for lk, lo, uk, up, ts in list(t.ranges())[::5]:
        c.scan.add(lk, lo, uk, up, (ts,))
    return c


def _nosst(bs):
    """A database that never flushed: runs of 200 and 65 entries, no SST at all."""
    rng = np.random.default_rng(37)
    v = lc.View("none", [], [], [], [], [])
    fresh = lambda: lc.gen_keys(rng, 1)[0]
    r0 = _exact(rng, 200, set(), [], fresh, [(b"ab", 1200, b"v-ab"), (b"abc", 1201, b"v-abc")])
    r1 = _exact(rng, 65, set(), [k for k, _, _ in r0], fresh)
    c = _new("nosst", bs, v, [r0, r1])
    point_queries(c, rng, [(q, TS_MAX) for q in (b"a", b"ab", b"abb", b"abc", b"abd")])
    gen_mem_ranges(c, rng, 0)
    return c


BUILDERS = {"mixed3": _mixed3, "ties2": _ties2, "many67": _many67, "nmem64": _nmem64, "one": _one, "allempty": _allempty,
            "nosst": _nosst}
CASES = (("mixed3", 128), ("ties2", 128), ("many67", 128), ("nmem64", 128), ("one", 128), ("allempty", 128), ("nosst", 0))


@lru_cache(maxsize=None)
def case(name, bs):
    return BUILDERS[name](bs)


def without_runs(c):
    """The case with nmem == 0."""
    return MemCase(c.name, c.bs, c.view, [], c.keys, c.read_ts, c.scan)


@lru_cache(maxsize=None)
def get_rows(name, bs, mode):
    c = case(name, bs)
    return [closed_get(c, k, ts, mode) for k, ts in zip(c.keys, c.read_ts)]


@lru_cache(maxsize=None)
def scan_rows(name, bs, mode):
    c = case(name, bs)
    return [closed_scan(c, lk, lo, uk, up, mode, ts) for lk, lo, uk, up, ts in c.scan.ranges()]


def get_arrays(c, rws):
    """Closed-form rows -> ({field: numpy array}, values list, val_off); val_pos absolute: a mem hit's
    into the runs' value arena, a table hit's into the files."""
    fo = c.view.file_off
    vo = c.stream()[3]
    out = {f: np.array([r[f] for r in rws], np.uint64) for f in GET_FIELDS if f != "val_pos"}
    pos = []
    for r in rws:
        if r["val_pos"] is None:
            pos.append(0)
        elif r["src"] < c.nmem:
            pos.append(int(vo[r["hit_ent"]]))
        else:
            pos.append(fo[r["sst"]] + r["val_pos"])
    out["val_pos"] = np.array(pos, np.uint64)
    values = [r["value"] for r in rws]
    val_off = np.concatenate([[0], np.cumsum([len(x) if x else 0 for x in values])]).astype(np.uint32)
    return out, values, val_off


@lru_cache(maxsize=None)
def get_expected(name, bs, mode):
    return get_arrays(case(name, bs), get_rows(name, bs, mode))


@lru_cache(maxsize=None)
def scan_expected(name, bs, mode):
    return ls.arrays(scan_rows(name, bs, mode))


def scan_mode_args(mode):
    """-> (flags, whether q_ts is passed)"""
    return {"default": 0, "mvcc": 2, "merged": 0, "newest": 4, "newest_merged": 4}[mode], not mode.endswith("merged")


# ------------------------------------------------------------------------------ coverage classifiers
GET_CLASSES = ("mem_mutable_immutable_two_tables", "mem_blind_table_sees", "mem_tombstone_over_table_value",
               "equal_ts_mem_wins", "three_versions_read_between", "below_first_key", "above_last_key", "image_tie",
               "prefix_of_landing", "extends_predecessor", "decider_mutable", "decider_immutable", "decider_table_after_runs",
               "newest_table_beats_run", "table_src_ge_64")


@lru_cache(maxsize=None)
def get_classes(name, bs):
    c = case(name, bs)
    n = dict.fromkeys(GET_CLASSES, 0)
    d, w = get_rows(name, bs, "mvcc"), get_rows(name, bs, "newest")
    for i, (key, ts) in enumerate(zip(c.keys, c.read_ts)):
        r, x = d[i], w[i]
        t = lc.closed(c.view, key, ts, "mvcc")
        tw = lc.closed(c.view, key, ts, "newest")
        inrun = [any(e[0] == key for e in run) for run in c.runs]
        n["mem_mutable_immutable_two_tables"] += bool(inrun and inrun[0] and any(inrun[1:]) and len(holders(c.view, key)) >= 2)
        mem_dec = r["src"] != NONE and r["src"] < c.nmem
        n["mem_blind_table_sees"] += mem_dec and r["status"] == ABSENT and t["status"] == FOUND
        n["mem_tombstone_over_table_value"] += mem_dec and r["status"] == TOMBSTONE and t["status"] == FOUND
        n["equal_ts_mem_wins"] += x["src"] != NONE and x["src"] < c.nmem and tw["src"] != NONE and tw["ts"] == x["ts"]
        n["decider_mutable"] += r["src"] == 0 and c.nmem > 0
        n["decider_immutable"] += mem_dec and r["src"] > 0
        n["decider_table_after_runs"] += c.nmem > 0 and r["src"] != NONE and r["src"] >= c.nmem
        n["newest_table_beats_run"] += x["src"] != NONE and x["src"] >= c.nmem and any(
            mem_lookup(run, key, ts)[1] is not None for run in c.runs)
        n["table_src_ge_64"] += c.nmem > 0 and r["src"] != NONE and r["src"] >= 64
        for run in c.runs:
            if not run:
                continue
            keys = run_keys(run)
            n["below_first_key"] += key < keys[0]
            n["above_last_key"] += key > keys[-1]
            p = bisect.bisect_left(keys, key)
            vers = [e for e in run if e[0] == key]
            n["three_versions_read_between"] += len(vers) >= 3 and vers[0][1] > ts >= vers[-1][1]
            n["image_tie"] += any(gc.image(k) == gc.image(key) and k != key for k in keys[max(p - 1, 0):p + 2])
            n["prefix_of_landing"] += p < len(keys) and keys[p] != key and keys[p].startswith(key)
            n["extends_predecessor"] += p > 0 and key.startswith(keys[p - 1]) and keys[p - 1] != key
    return {k: int(v) for k, v in n.items()}


SCAN_CLASSES = ("excluded_lower_on_multi_version_key", "included_upper_on_multi_version_key", "slice_empty", "slice_one",
                "slice_whole_run", "overlap_fails_below", "overlap_fails_above", "over_64_runs", "mem_and_table_runs",
                "mem_owner_hides_table", "key_in_two_mem_runs") + tuple("kinds_%d%d" % (a, b) for a in KINDS for b in KINDS)


@lru_cache(maxsize=None)
def scan_classes(name, bs):
    c = case(name, bs)
    n = dict.fromkeys(SCAN_CLASSES, 0)
    multi = {a[0] for run in c.runs for a, b in zip(run, run[1:]) if a[0] == b[0]}
    for lk, lo, uk, up, ts in c.scan.ranges():
        if bad_range(lk, lo, uk, up):
            continue
        n["kinds_%d%d" % (lk, uk)] += 1
        n["excluded_lower_on_multi_version_key"] += lk == EXCLUDED and lo in multi
        n["included_upper_on_multi_version_key"] += uk == INCLUDED and up in multi
        mem_keys, nmem_runs = [], 0
        for run in c.runs:
            if not run:
                continue
            n["overlap_fails_below"] += bool(uk) and not mem_passes(run, UNBOUNDED, b"", uk, up)
            n["overlap_fails_above"] += bool(lk) and not mem_passes(run, lk, lo, UNBOUNDED, b"")
            if mem_passes(run, lk, lo, uk, up):
                b, e = mem_slice(run, lk, lo, uk, up)
                nmem_runs += 1
                mem_keys.append({x[0] for x in run[b:e]})
                n["slice_empty"] += e == b
                n["slice_one"] += e - b == 1
                n["slice_whole_run"] += e - b == len(run) and len(run) > 1
        runs = runs_of(c, lk, lo, uk, up, True)
        n["over_64_runs"] += nmem_runs > 0 and len(runs) > 64
        tab_keys = {e[0] for r in runs[nmem_runs:] for e in r}
        n["mem_and_table_runs"] += nmem_runs > 0 and len(runs) > nmem_runs
        n["mem_owner_hides_table"] += any(s & tab_keys for s in mem_keys)
        n["key_in_two_mem_runs"] += any(a & b for i, a in enumerate(mem_keys) for b in mem_keys[i + 1:])
    return {k: int(v) for k, v in n.items()}
