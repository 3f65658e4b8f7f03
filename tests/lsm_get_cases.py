"""LSM views and point reads that reach chosen paths of lsm_get_kernel -- TEST INFRASTRUCTURE.

The method of get_cases.py / scan_cases.py for lsmblk_lsm_get_batch; shared by test_lsm_get_cases.py
(CPU: two independent routes to every expectation, and the generators reach what they were built
for) and test_gpu_lsm_get.py (GPU: every result field against the expectation).

  tables        get_cases.make_sst (pyref.sst_file)
  closed form   closed(): per source get_cases.lookup, the decider rule / the NEWEST maximum
  line by line  line_by_line(): keep_table, SsTableIterator / SstConcatIterator seeks as entry runs,
                pyref.MergeIterator over them in priority order, scan_cases.LsmIterator(.., Unbounded,
                read_ts), `key == query and value` (get_with_ts, src/lsm_storage.rs:361-439, with the
                one MergeIterator of LSMBLK_MERGE_RUNS in place of the TwoMergeIterator nesting)
  newest_plain  a plain maximum over every version of the key in every table that passes keep_table
"""
import bisect
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import get_cases as gc
import scan_cases as sc
from oracle import pyref

NONE = gc.NONE
ABSENT, FOUND, TOMBSTONE, RANGE_OUT, BLOOM_OUT = gc.ABSENT, gc.FOUND, gc.TOMBSTONE, gc.RANGE_OUT, gc.BLOOM_OUT
FIELDS = ("status", "src", "sst", "hit_blk", "hit_ent", "vlen", "ts", "val_pos", "seeks", "bloom_out")
MODES = ("default", "mvcc", "newest")
FLAGS = {"default": 0, "mvcc": 2, "newest": 4}  # LSMBLK_GET_MVCC, LSMBLK_LSM_GET_NEWEST
KARY = 64  # kary_first_false's probes per step (lsmblk_get.hip)

_fp = {}


def fp(key):
    if key not in _fp:
        _fp[key] = pyref.fingerprint32(key)
    return _fp[key]


@dataclass
class View:
    name: str
    ssts: list      # get_cases.Sst, by SST id
    l0: list        # SST ids, priority order
    levels: list    # per level its SST ids in key order
    keys: list
    read_ts: list

    @property
    def files(self):
        return b"".join(s.buf for s in self.ssts)

    @property
    def file_off(self):
        return [0] + [int(x) for x in np.cumsum([len(s.buf) for s in self.ssts])]

    @property
    def nsrc(self):
        return len(self.l0) + len(self.levels)


def first_key(s):
    return s.first_keys[0]


def last_key(s):
    return s.metas[-1][2]


def keep_table(s, key):
    """keep_table of get_with_ts (src/lsm_storage.rs:383-398)."""
    return first_key(s) <= key <= last_key(s) and s.bloom.may_contain(fp(key))


# ------------------------------------------------------------------------------ (a) the closed form
def source_table(v, src, key):
    """The SST id source `src` offers for the key, or None (a level: the last table with first_key <= key)."""
    if src < len(v.l0):
        return v.l0[src]
    lv = v.levels[src - len(v.l0)]
    p = bisect.bisect_right([first_key(v.ssts[t]) for t in lv], key)
    return lv[p - 1] if p else None


def on_key(s, r, key):
    b, e = r["blk"], r["ent"]
    return b != NONE and b < len(s.blocks) and s.blocks[b][e][0] == key


def closed(v, key, read_ts, mode):
    """One key -> the result record's fields (val_pos relative to the table's file) and the value."""
    out = dict(status=ABSENT, src=NONE, sst=NONE, hit_blk=NONE, hit_ent=NONE, vlen=0, ts=0, val_pos=None, value=None)
    seeks = bloom_out = 0
    if key:
        for src in range(v.nsrc):
            t = source_table(v, src, key)
            if t is None:
                continue
            r = gc.lookup(v.ssts[t], key, read_ts, False, mode != "default", fp)
            if r["status"] == RANGE_OUT:
                continue
            if r["status"] == BLOOM_OUT:
                bloom_out += 1
                continue
            seeks += 1
            pick = dict(status=r["status"], src=src, sst=t, hit_blk=r["hit_blk"], hit_ent=r["hit_ent"], vlen=r["vlen"],
                        ts=r["ts"], val_pos=r["val_pos"], value=r["value"])
            if mode != "newest":
                if on_key(v.ssts[t], r, key):
                    out = pick
                    break
            elif r["status"] != ABSENT and (out["src"] == NONE or r["ts"] > out["ts"]):
                out = pick
    return dict(out, seeks=seeks, bloom_out=bloom_out)


# ------------------------------------------------------------------------------ (b) line by line
def flat(s):
    """(entries of the table in order, index of every block's first entry)"""
    if not hasattr(s, "_flat"):
        s._flat = [(k, ts, val) for blk in s.blocks for k, ts, val, _ in blk]
        s._start = [0] + [int(x) for x in np.cumsum([len(b) for b in s.blocks])]
    return s._flat, s._start


class Run(pyref.ListIter):
    """pyref.ListIter over the entries of consecutive tables from a position on, without copying them:
    an SsTableIterator after its seek (one table), or an SstConcatIterator (the tables that follow)."""

    def __init__(self, parts):  # [(entries, first index)]
        self.parts = [(e, i) for e, i in parts]
        self.p = 0
        self._skip()

    def _skip(self):
        while self.p < len(self.parts) and self.parts[self.p][1] >= len(self.parts[self.p][0]):
            self.p += 1

    def is_valid(self):
        return self.p < len(self.parts)

    def entry(self):
        e, i = self.parts[self.p]
        return e[i]

    def key(self):
        return self.entry()[0]

    def next(self):
        e, i = self.parts[self.p]
        self.parts[self.p] = (e, i + 1)
        self._skip()


def table_seek(s, key, mvcc):
    """SsTableIterator::create_and_seek_to_key -> (entries, index of the landing)"""
    e, start = flat(s)
    b, x = gc.seek_to_key_inner(s, key, mvcc)
    return e, start[b] + x


def concat_seek(tables, key, mvcc):
    """SstConcatIterator::create_and_seek_to_key (src/iterators/concat_iterator.rs:50-80)."""
    idx = max(bisect.bisect_right([first_key(s) for s in tables], key) - 1, 0)
    if idx >= len(tables):
        return Run([])
    return Run([table_seek(tables[idx], key, mvcc)] + [(flat(s)[0], 0) for s in tables[idx + 1:]])


def line_by_line(v, key, read_ts, mvcc):
    """get_with_ts over the view -> (value, ts) or None."""
    iters = [Run([table_seek(v.ssts[t], key, mvcc)]) for t in v.l0 if keep_table(v.ssts[t], key)]
    for lv in v.levels:
        iters.append(concat_seek([v.ssts[t] for t in lv if keep_table(v.ssts[t], key)], key, mvcc))
    it = sc.LsmIterator(pyref.MergeIterator(iters), (sc.UNBOUNDED, b""), read_ts)
    if it.is_valid() and it.entry()[0] == key and it.entry()[2]:
        return it.entry()[2], it.entry()[1]
    return None


def newest_plain(v, key, read_ts):
    """(ts, source ordinal, value) of the newest version <= read_ts over every table that passes
    keep_table (the lower ordinal wins an equal ts), or None."""
    best = None
    tabs = [(i, t) for i, t in enumerate(v.l0)] + [(len(v.l0) + l, t) for l, lv in enumerate(v.levels) for t in lv]
    for src, t in tabs:
        s = v.ssts[t]
        if not keep_table(s, key):
            continue
        for k, ts, val in flat(s)[0]:
            if k == key and ts <= read_ts and (best is None or ts > best[0]):
                best = (ts, src, val)
    return best


# ------------------------------------------------------------------------------ generators
def gen_keys(rng, n, alphabet=b"abcd", klen=(1, 9), prefix=b""):
    keys = set()
    while len(keys) < n:
        keys.add(prefix + bytes(rng.choice(list(alphabet), int(rng.integers(*klen))).astype(np.uint8)))
    return sorted(keys)


def gen_versions(rng, keys, maxver=4, tomb=0.25, vlen=(1, 40)):
    out = []
    for k in keys:
        tss = sorted({int(t) for t in rng.integers(1, 1000, int(rng.integers(1, maxver + 1)))}, reverse=True)
        for ts in tss:
            val = b"" if rng.random() < tomb else bytes(rng.integers(0, 256, int(rng.integers(*vlen)), dtype=np.uint8))
            out.append((k, ts, val))
    return out


def split(entries, parts):
    """The entries in `parts` runs of whole keys (a level's tables)."""
    keys = sorted({k for k, _, _ in entries})
    cut = [keys[len(keys) * i // parts] for i in range(1, parts)]
    runs = [[] for _ in range(parts)]
    for e in entries:
        runs[bisect.bisect_right(cut, e[0])].append(e)
    return runs


def pick(rng, pool, n):
    return sorted(pool[i] for i in rng.choice(len(pool), n, replace=False))


def read_ts_of(rng, n):
    out = []
    for _ in range(n):
        out += [0, int(rng.integers(1, 1000)), int(rng.integers(1, 1000)), 1 << 60]
    return out


def _mixed(bs, seed=11):
    """3 L0 tables of 150 keys over one pool (overlapping ranges), the first two with one version per
    key -- 10 filter bits per key, the reference's ~1 % false positives -- the third with up to 4;
    level 0 of 3 and level 1 of 4 tables split from 300-key sets of the pool's middle, so keys of the
    view lie below, above and between a level's tables."""
    rng = np.random.default_rng(seed)
    pool = gen_keys(rng, 900)
    ssts, l0, levels = [], [], []
    for i, (lo, hi, maxver) in enumerate(((120, 780, 1), (0, 900, 1), (60, 840, 4))):
        l0.append(len(ssts))
        ssts.append(gc.make_sst(gen_versions(rng, pick(rng, pool[lo:hi], 150), maxver=maxver), bs))
    for parts, trim in ((3, 30), (4, 60)):
        lv = []
        for run in split(gen_versions(rng, pick(rng, pool[trim:-trim], 300), maxver=4), parts):
            lv.append(len(ssts))
            ssts.append(gc.make_sst(run, bs))
        levels.append(lv)
    pool = sorted({k for s in ssts for k, _, _ in s.entries})  # every key of the view
    have = set(pool)
    absent = set()
    while len(absent) < 200:
        k = pool[int(rng.integers(len(pool)))]
        c = k + bytes([int(rng.integers(97, 102))]) if rng.random() < 0.6 else k[:-1]
        if c and c not in have:
            absent.add(c)
    keys = pool + sorted(absent) + [b"A", b"\x00", b"a", b"zz", pool[-1] + b"\xff"]
    qk = [k for k in keys for _ in range(4)]
    return View("mixed", ssts, l0, levels, qk, read_ts_of(rng, len(keys)))


LEVEL_SIZES = (1, 3, 0, KARY, KARY + 1, KARY + 6)  # an empty level between two; 65 and 70 cross the 64-probe step
_num = lambda x: b"k%06d" % x


def _levels(bs, seed=8):
    """Tiny tables (2-4 entries) over one key space, 100 numbers per table slot with a gap after each."""
    rng = np.random.default_rng(seed)
    ssts, levels, keys = [], [], []
    l0 = [0]
    ssts.append(gc.make_sst(gen_versions(rng, [_num(100 * i + 50) for i in range(0, 70, 7)], maxver=2), bs))
    for n in LEVEL_SIZES:
        lv = []
        for j in range(n):
            first = 100 * j + 10 * int(rng.integers(1, 4))
            ks = [_num(first + 10 * i) for i in range(int(rng.integers(1, 4)))]
            ents = gen_versions(rng, ks, maxver=2 if len(ks) > 1 else 3)
            if len(ents) < 2:
                ents.append((ks[0], 0, b"v0"))
            ents = ents[:4]
            lv.append(len(ssts))
            ssts.append(gc.make_sst(ents, bs))
            fk, lk = int(ents[0][0][1:]), int(ents[-1][0][1:])
            keys += [_num(fk), _num(lk), _num(fk - 1), _num(lk + 1), _num(100 * j + 95)]
        levels.append(lv)
    keys = sorted(set(keys)) + [_num(0), _num(100 * (KARY + 6) + 5), b"j", b"l"]
    ts = [int(rng.choice([0, int(rng.integers(1, 1000)), 1 << 60])) for _ in keys]
    return View("levels", ssts, l0, levels, keys, ts)


TIE_PREFIX = gc.TIE_PREFIX  # 20 bytes, longer than the image


def _ties(bs, seed=9):
    rng = np.random.default_rng(seed)
    ssts, levels = [], []
    a = gen_versions(rng, gen_keys(rng, 120, prefix=TIE_PREFIX, klen=(1, 7)))
    b = gen_versions(rng, gen_keys(rng, 100, prefix=TIE_PREFIX[:gc.IMG_BYTES - 2], klen=(1, 6)))
    l0 = [0]
    ssts.append(gc.make_sst(gen_versions(rng, pick(rng, sorted({k for k, _, _ in a + b}), 40), maxver=1), bs))
    for ents, parts in ((a, 6), (b, 5)):
        lv = []
        for run in split(ents, parts):
            lv.append(len(ssts))
            ssts.append(gc.make_sst(run, bs))
        levels.append(lv)
    keys = sorted({k for k, _, _ in a + b})
    keys += [k + b"b" for k in keys[::3]] + [k[:-1] for k in keys[::4]]
    keys += [TIE_PREFIX, TIE_PREFIX[:gc.IMG_BYTES], TIE_PREFIX[:gc.IMG_BYTES] + b"\x00", TIE_PREFIX + b"zzzz"]
    ts = [int(rng.choice([0, int(rng.integers(1, 1000)), int(rng.integers(1, 1000)), 1 << 60])) for _ in keys]
    return View("ties", ssts, l0, levels, keys, ts)


def _edges(kind, bs):
    m = _mixed(bs, seed=10)
    keys, ts = m.keys[::5], m.read_ts[::5]
    if kind == "edges_one64":  # one level of exactly 64 tables: all of them routed by one probe each
        lv = _levels(bs)
        return View(kind, lv.ssts, [], [lv.levels[3]], lv.keys, lv.read_ts)
    if kind == "edges_72_sources":  # more sources than lanes: 70 L0 tables, then two levels in the second 64
        lv = _levels(bs)
        return View(kind, lv.ssts, lv.levels[5], [lv.levels[3], lv.levels[4]], lv.keys, lv.read_ts)
    if kind == "edges_levels":
        return View(kind, m.ssts, [], m.levels, keys, ts)
    if kind == "edges_l0":
        return View(kind, m.ssts, m.l0, [], keys, ts)
    return View(kind, m.ssts, [], [], keys, ts)


def _threshold(bs, seed=11):
    """get_cases.threshold_entries() as an L0 table behind an ordinary one and above a level: its
    blocks on both sides of kGetLdsBlock are read as a non-first source."""
    rng = np.random.default_rng(seed)
    big = gc.threshold_entries()
    ordinary = gen_versions(rng, gen_keys(rng, 100) + [b"b-at", b"e-run"], maxver=3)
    ordinary.sort(key=lambda e: e[0])  # (stable: a key's versions stay newest first)
    level = split(gen_versions(rng, gen_keys(rng, 120) + [b"c-over", b"d-huge"], maxver=2), 2)
    for run in level:
        run.sort(key=lambda e: e[0])
    ssts = [gc.make_sst(ordinary, bs), gc.make_sst(big, bs)] + [gc.make_sst(run, bs) for run in level]
    keys = sorted({k for s in ssts for k, _, _ in s.entries})
    ts = [int(rng.choice([0, 4, 8, int(rng.integers(1, 1000)), 1 << 60])) for _ in keys]
    for k in (b"b-at", b"c-over", b"d-huge", b"e-run"):  # every version boundary of the large entries
        for t in (0, 2, 3, 4, 5, 8, 9, 29, 30, 39, 40, 49, 50, 99):
            keys.append(k)
            ts.append(t)
    return View("threshold", ssts, [0, 1], [[2, 3]], keys, ts)


CASES = (("mixed", 128), ("mixed", 256), ("levels", 128), ("levels", 256), ("ties", 128), ("ties", 256),
         ("edges_levels", 128), ("edges_l0", 256), ("edges_empty", 128), ("edges_one64", 128), ("edges_72_sources", 128),
         ("threshold", 4096))


@lru_cache(maxsize=None)
def case(name, bs):
    if name == "mixed":
        return _mixed(bs)
    if name == "levels":
        return _levels(bs)
    if name == "ties":
        return _ties(bs)
    if name.startswith("edges"):
        return _edges(name, bs)
    if name == "threshold":
        return _threshold(bs)
    raise KeyError(name)


@lru_cache(maxsize=None)
def rows(name, bs, mode):
    v = case(name, bs)
    return [closed(v, k, ts, mode) for k, ts in zip(v.keys, v.read_ts)]


def arrays(v, rws):
    """Closed-form rows -> ({field: numpy array}, values list, val_off); val_pos absolute."""
    fo = v.file_off
    out = {f: np.array([r[f] for r in rws], np.uint64) for f in FIELDS if f != "val_pos"}
    out["val_pos"] = np.array([0 if r["val_pos"] is None else fo[r["sst"]] + r["val_pos"] for r in rws], np.uint64)
    values = [r["value"] for r in rws]
    val_off = np.concatenate([[0], np.cumsum([len(x) if x else 0 for x in values])]).astype(np.uint32)
    return out, values, val_off


@lru_cache(maxsize=None)
def expected(name, bs, mode):
    return arrays(case(name, bs), rows(name, bs, mode))


# ------------------------------------------------------------------------------ coverage classifiers
CLASSES = ("decider_src0", "decider_later_l0", "decider_level", "earlier_false_positive", "earlier_bloom_out",
           "earlier_range_out", "decider_blind_later_sees", "default_mvcc_differ", "mvcc_newest_differ", "tombstone",
           "level_gap", "level_below", "level_above", "image_tie", "level_over_64", "big_block_later_source")


def searched(v, key, mode, upto):
    """Per source before `upto`: (src, table or None, get_cases.lookup's record)."""
    out = []
    for src in range(min(upto, v.nsrc)):
        t = source_table(v, src, key)
        out.append((src, t, gc.lookup(v.ssts[t], key, 0, False, mode != "default", fp) if t is not None else None))
    return out


@lru_cache(maxsize=None)
def classes(name, bs):
    v = case(name, bs)
    n = dict.fromkeys(CLASSES, 0)
    d, m, w = rows(name, bs, "default"), rows(name, bs, "mvcc"), rows(name, bs, "newest")
    nl0 = len(v.l0)
    for i, (key, ts) in enumerate(zip(v.keys, v.read_ts)):
        r = d[i]
        if r["src"] != NONE:
            n["decider_src0"] += r["src"] == 0
            n["decider_later_l0"] += 0 < r["src"] < nl0
            n["decider_level"] += r["src"] >= nl0
            before = searched(v, key, "default", r["src"])
            n["earlier_false_positive"] += any(x is not None and x["status"] == ABSENT for _, _, x in before)
            n["earlier_bloom_out"] += any(x is not None and x["status"] == BLOOM_OUT for _, _, x in before)
            n["earlier_range_out"] += any(x is not None and x["status"] == RANGE_OUT for _, _, x in before)
            if r["status"] == ABSENT:
                later = [closed(View("", v.ssts, [t], [], [], []), key, ts, "default")
                         for s2, t, _ in searched(v, key, "default", v.nsrc)[r["src"] + 1:] if t is not None]
                n["decider_blind_later_sees"] += any(x["status"] != ABSENT for x in later)
        x = m[i]  # (the corrected landing: the reference's lands past a key's first, oversized, block)
        if x["src"] not in (0, NONE) and x["hit_blk"] != NONE:
            tab = v.ssts[x["sst"]]
            n["big_block_later_source"] += tab.ends[x["hit_blk"]] - 4 - tab.metas[x["hit_blk"]][0] > gc.kGetLdsBlock
        n["default_mvcc_differ"] += any(d[i][f] != m[i][f] for f in FIELDS)
        n["mvcc_newest_differ"] += any(m[i][f] != w[i][f] for f in ("status", "ts", "sst", "hit_blk", "hit_ent"))
        n["tombstone"] += r["status"] == TOMBSTONE
        for lv in v.levels:
            if not lv:
                continue
            firsts = [first_key(v.ssts[t]) for t in lv]
            p = bisect.bisect_right(firsts, key)
            n["level_below"] += p == 0
            n["level_above"] += p == len(lv) and key > last_key(v.ssts[lv[-1]])
            n["level_gap"] += 0 < p < len(lv) and key > last_key(v.ssts[lv[p - 1]])
            n["level_over_64"] += len(lv) > KARY and p > 0
            ties = [j for j, fk in enumerate(firsts) if gc.image(fk) == gc.image(key)]
            n["image_tie"] += len({firsts[j] for j in ties}) >= 3 and p > 0 and ties[0] < p - 1 < ties[-1]
    return {k: int(x) for k, x in n.items()}
