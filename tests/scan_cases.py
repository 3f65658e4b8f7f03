"""SST sets and range scans that reach chosen paths of the scan kernels (lsmblk_get.hip) and of the
read filter (lsmblk_gpu.hip) -- TEST INFRASTRUCTURE.

The method of get_cases.py for the batched range read (lsmblk_sst_scan_batch,
lsmblk_read_filter_batch); shared by test_scan_cases.py (CPU: the generators reach what they were
built for, the read filter's closed form equals the loop) and test_gpu_scan.py (GPU: every result
field and every output byte against the expectation).

  files         get_cases.make_sst (pyref.sst_file); the SSTs of the get cases
  expectations  range_overlap (src/lsm_storage.rs:142-167), the begin rule of scan_with_ts
                (:482-498) over get_cases.seek_to_key_inner with SsTableIterator::next, the end
                bound as a plain walk over entries, and LsmIterator (src/lsm_iterator.rs:20-113)
                as a class over a list iterator, all restated below
  constants     kGetLdsBlock, kScanWg, kFiltTile read out of the kernel sources
"""
import bisect
import os
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import get_cases as gc
import path_cases as pc
from oracle import pyref

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsm_amd", "csrc")
kGetLdsBlock = gc.kGetLdsBlock
kScanWg = pc.read_constants(os.path.join(_CSRC, "lsmblk_get.hip"), ("kScanWg",))["kScanWg"]
kFiltTile = pc.read_constants(os.path.join(_CSRC, "lsmblk_gpu.hip"), ("kFiltTile",))["kFiltTile"]

UNBOUNDED, INCLUDED, EXCLUDED = 0, 1, 2
OK, EMPTY, RANGE_OUT = 0, 1, 2
NONE = gc.NONE
FIELDS = ("status", "blk0", "ent0", "blk1", "ent1", "blocks", "n")
MODES = gc.MODES  # (no_filter, mvcc)
KINDS = (UNBOUNDED, INCLUDED, EXCLUDED)


# ------------------------------------------------------------------------------ the scan, restated
def range_overlap(lk, lower, uk, upper, table_begin, table_end):
    """range_overlap (src/lsm_storage.rs:142-167)."""
    if uk == EXCLUDED and upper <= table_begin:
        return False
    if uk == INCLUDED and upper < table_begin:
        return False
    if lk == EXCLUDED and lower >= table_end:
        return False
    if lk == INCLUDED and lower > table_end:
        return False
    return True


def sst_next(s, b, e):
    """SsTableIterator::next (src/table/iterator.rs:86-97): the next entry, at a block's end entry 0
    of the next block; blk == the block count: invalid."""
    e += 1
    if e == len(s.blocks[b]):
        b, e = b + 1, 0
    return b, e


def begin(s, lk, lower, mvcc):
    """The iterator scan_with_ts builds for one table (src/lsm_storage.rs:482-498) -> (blk, ent)."""
    if lk == UNBOUNDED:
        return 0, 0  # create_and_seek_to_first
    b, e = gc.seek_to_key_inner(s, lower, mvcc)
    if lk == EXCLUDED:
        while b < len(s.blocks) and s.blocks[b][e][0] == lower:  # :492-494
            b, e = sst_next(s, b, e)
    return b, e


def scan_one(s, lk, lower, uk, upper, no_filter, mvcc):
    """One range -> the result record's fields and the entries [(key, ts, value)] of [begin, end).
    The end bound is tested on every entry from begin on, the first included."""
    if (lk and not lower) or (uk and not upper):
        return dict(status=EMPTY, blk0=NONE, ent0=NONE, blk1=NONE, ent1=NONE, blocks=0, n=0, entries=[])
    if not no_filter and not range_overlap(lk, lower, uk, upper, s.first_keys[0], s.metas[-1][2]):
        return dict(status=RANGE_OUT, blk0=NONE, ent0=NONE, blk1=NONE, ent1=NONE, blocks=0, n=0, entries=[])
    b0, e0 = begin(s, lk, lower, mvcc)
    b, e, ents, touched = b0, e0, [], set()
    while b < len(s.blocks):
        k, ts, v, _ = s.blocks[b][e]
        if (uk == INCLUDED and not k <= upper) or (uk == EXCLUDED and not k < upper):
            break
        ents.append((k, ts, v))
        touched.add(b)
        b, e = sst_next(s, b, e)
    return dict(status=OK if ents else EMPTY, blk0=b0, ent0=e0, blk1=b, ent1=e, blocks=len(touched), n=len(ents),
                entries=ents)


class LsmIterator:
    """LsmIterator (src/lsm_iterator.rs:20-113), line by line, over a pyref.ListIter-like inner
    iterator; end_bound = (kind, key)."""

    def __init__(self, inner, end_bound, read_ts):  # new, :29-43 (the first position is not tested)
        self.inner, self.end_bound, self.read_ts = inner, end_bound, read_ts
        self.valid = inner.is_valid()
        self.prev_key = b""
        self.move_to_key()

    def next_inner(self):  # :45-57
        self.inner.next()
        if not self.inner.is_valid():
            self.valid = False
            return
        kind, key = self.end_bound
        if kind == INCLUDED:
            self.valid = self.inner.entry()[0] <= key
        elif kind == EXCLUDED:
            self.valid = self.inner.entry()[0] < key

    def move_to_key(self):  # :59-86
        while True:
            while self.inner.is_valid() and self.inner.entry()[0] == self.prev_key:
                self.next_inner()
            if not self.inner.is_valid():
                break
            self.prev_key = self.inner.entry()[0]
            while (self.inner.is_valid() and self.inner.entry()[0] == self.prev_key
                   and self.inner.entry()[1] > self.read_ts):
                self.next_inner()
            if not self.inner.is_valid():
                break
            if self.inner.entry()[0] != self.prev_key:
                continue
            if self.inner.entry()[2]:
                break

    def is_valid(self):
        return self.valid

    def entry(self):
        return self.inner.entry()

    def next(self):  # :104-108
        self.next_inner()
        self.move_to_key()


def lsm_iterate(entries, read_ts, end_bound=(UNBOUNDED, b"")):
    """What FusedIterator<LsmIterator> yields over `entries`."""
    it, out = LsmIterator(pyref.ListIter(entries), end_bound, read_ts), []
    while it.is_valid():
        out.append(it.entry())
        it.next()
    return out


def read_filter_rule(entries, read_ts):
    """The predecessor-only closed form of lsmblk_read_filter_batch over one segment."""
    out = []
    for i, (k, ts, v) in enumerate(entries):
        if ts <= read_ts and v and (i == 0 or entries[i - 1][0] != k or entries[i - 1][1] > read_ts):
            out.append((k, ts, v))
    return out


# ------------------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    ssts: list
    q_sst: list
    lower: list
    upper: list
    lkind: list
    ukind: list

    @property
    def files(self):
        return b"".join(s.buf for s in self.ssts)

    @property
    def file_off(self):
        return [0] + list(np.cumsum([len(s.buf) for s in self.ssts]))

    def add(self, si, lk, lower, uk, upper):
        self.q_sst.append(si)
        self.lkind.append(lk)
        self.lower.append(lower if lk else b"")
        self.ukind.append(uk)
        self.upper.append(upper if uk else b"")

    def __len__(self):
        return len(self.q_sst)


def bound_pool(s, rng):
    """Sorted candidate bound keys: present keys, keys shortened by a byte, keys with a byte
    appended, below the first key and above the last."""
    keys = sorted({k for k, _, _ in s.entries})
    pool = set(keys) | {k[:-1] for k in keys if len(k) > 1}
    pool |= {k + bytes([int(rng.integers(97, 102))]) for k in keys[::3]}
    pool |= {b"\x01", keys[0][:1], keys[-1] + b"\xff", b"\xff\xff"}
    return sorted(pool), keys


def gen_ranges(c, si, seed, per_pair=36):
    s = c.ssts[si]
    rng = np.random.default_rng(seed)
    pool, keys = bound_pool(s, rng)
    for lk in KINDS:
        for uk in KINDS:
            for _ in range(per_pair):  # short ranges: the upper bound a few pool keys on
                i = int(rng.integers(0, len(pool)))
                j = min(i + int(rng.integers(0, 14)), len(pool) - 1)
                c.add(si, lk, pool[i], uk, pool[j])
            for _ in range(3):  # lower > upper
                i = int(rng.integers(1, len(pool)))
                c.add(si, lk, pool[i], uk, pool[int(rng.integers(0, i))])
            for _ in range(4):  # lower == upper, present and absent keys
                k = keys[int(rng.integers(0, len(keys)))] if rng.random() < 0.7 else pool[int(rng.integers(0, len(pool)))]
                c.add(si, lk, k, uk, k)
            c.add(si, lk, pool[0], uk, pool[-1])  # the whole table by its bounds
            c.add(si, lk, pool[len(pool) // 3], uk, pool[2 * len(pool) // 3])  # a long range


def _from_get(name, seed):
    g = gc.case(name)
    c = Case(name, g.ssts, [], [], [], [], [])
    for si in range(len(g.ssts)):
        gen_ranges(c, si, seed + si)
    return c


def distinct_starts(s):
    """Blocks whose first key differs from the previous block's last key: a lower bound Included(first
    key) lands on their entry 0 in both modes."""
    return [b for b in range(len(s.blocks)) if b == 0 or s.blocks[b - 1][-1][0] != s.blocks[b][0][0]]


MANY_TOUCH = (1, 2, 63, 64, 65, 130)
CASES = ("bs128", "bs256", "bs4096", "ties", "threshold", "many_blocks")


@lru_cache(maxsize=None)
def case(name):
    if name in ("bs128", "bs256", "bs4096"):
        return _from_get(name, {"bs128": 100, "bs256": 200, "bs4096": 300}[name])
    if name == "ties":
        c = _from_get(name, 400)
        T = gc.TIE_PREFIX
        for lk in KINDS:
            for uk in KINDS:
                for si in (0, 2):
                    c.add(si, lk, T[:gc.IMG_BYTES], uk, T + b"zzzz")
                    c.add(si, lk, T, uk, T[:gc.IMG_BYTES] + b"\x00")
        return c
    if name == "threshold":
        g = gc.case("threshold")
        c = Case(name, g.ssts, [], [], [], [], [])
        marks = [b"a038", b"a039", b"b-at", b"c-over", b"d-huge", b"e-run", b"f", b"g"]
        for lk in KINDS:
            for uk in KINDS:
                for i, lo in enumerate(marks):
                    for up in marks[i:]:
                        c.add(0, lk, lo, uk, up)
        gen_ranges(c, 1, 500, per_pair=8)
        # the get cases' large entries are all followed by a small version of their key, so no range
        # ends with one of their blocks: a third SST whose threshold blocks are their keys' only version
        big = lambda k, ts, size: (k, ts, bytes((len(k) + i) & 0xFF for i in range(size - 18 - len(k))))
        ents = [(b"m%02d" % i, 7, b"v%d" % i) for i in range(6)]
        ents += [big(b"n-at", 9, kGetLdsBlock), big(b"o-over", 9, kGetLdsBlock + 1), big(b"p-huge", 9, 3 * kGetLdsBlock)]
        ents += [(b"q", 4, b"z"), (b"q", 2, b"")]
        c.ssts = c.ssts + [gc.make_sst(ents, 4096)]
        marks = [b"m04", b"m05", b"n-at", b"o-over", b"p-huge", b"q", b"r"]
        for lk in KINDS:
            for uk in KINDS:
                for i, lo in enumerate(marks):
                    for up in marks[i:]:
                        c.add(2, lk, lo, uk, up)
        return c
    if name == "many_blocks":
        s = gc.make_sst(gc.gen_entries(61, nkeys=700), 128)
        assert len(s.blocks) >= 200
        c = Case(name, [s], [], [], [], [], [])
        ds = distinct_starts(s)
        rng = np.random.default_rng(600)
        for t in MANY_TOUCH:  # Included(first key of b) .. Excluded(first key of b + t): exactly t blocks
            cand = [b for b in ds if b + t in ds]
            for b in (cand[0], cand[len(cand) // 2], cand[-1]):
                c.add(0, INCLUDED, s.first_keys[b], EXCLUDED, s.first_keys[b + t])
        c.add(0, UNBOUNDED, b"", UNBOUNDED, b"")
        gen_ranges(c, 0, 601, per_pair=12)
        base = len(c)
        while len(c) < kScanWg + 1:  # repeated ranges, each written in full: the scans' round edges
            i = int(rng.integers(len(MANY_TOUCH) * 3 + 1, base))
            c.add(0, c.lkind[i], c.lower[i], c.ukind[i], c.upper[i])
        return c
    raise KeyError(name)


def query_counts():
    """Queries per call at the edges of a wave and of the one-workgroup scans' shares."""
    return (1, 63, 64, 65, kScanWg - 1, kScanWg, kScanWg + 1)


def stream_of(rows):
    """Per-range entry lists -> (keys bytes, key_off, vals bytes, val_off, ts, seg_start)."""
    ents = [e for r in rows for e in r]
    ko = np.concatenate([[0], np.cumsum([len(k) for k, _, _ in ents])]).astype(np.uint32)
    vo = np.concatenate([[0], np.cumsum([len(v) for _, _, v in ents])]).astype(np.uint32)
    seg = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    return (b"".join(k for k, _, _ in ents), ko, b"".join(v for _, _, v in ents), vo,
            np.array([t for _, t, _ in ents], np.uint64), seg)


@lru_cache(maxsize=None)
def expected(name, no_filter, mvcc):
    """Every range of the case -> ({field: numpy array}, per-range entry lists)."""
    c = case(name)
    memo, rows = {}, []
    for q in zip(c.q_sst, c.lkind, c.lower, c.ukind, c.upper):
        if q not in memo:
            memo[q] = scan_one(c.ssts[q[0]], q[1], q[2], q[3], q[4], no_filter, mvcc)
        rows.append(memo[q])
    out = {f: np.array([r[f] for r in rows], np.uint64) for f in FIELDS}
    return out, [r["entries"] for r in rows]


def read_ts_values(c):
    """0, the smallest, a middle and the largest timestamp of the case's SSTs, and 1 << 60."""
    tss = sorted({ts for s in c.ssts for _, ts, _ in s.entries})
    return (0, tss[0], tss[len(tss) // 2], tss[-1], 1 << 60)


# ------------------------------------------------------------------------------ coverage classifiers
CLASSES = ("range_out", "lower_gt_upper", "begin_differs", "begin_spill", "excl_cross", "end_ent0", "end_sst_end",
           "one_block", "ge65_blocks", "big_first", "big_last", "end_image_tie")


def classes(name, no_filter, mvcc):
    """Counts of the input classes the case reaches in one mode."""
    c = case(name)
    exp, _ = expected(name, no_filter, mvcc)
    other, _ = expected(name, no_filter, not mvcc)
    n = dict.fromkeys(CLASSES, 0)
    for i, (si, lk, lo, uk, up) in enumerate(zip(c.q_sst, c.lkind, c.lower, c.ukind, c.upper)):
        s = c.ssts[si]
        st, b0, e0, b1, e1 = (int(exp[f][i]) for f in ("status", "blk0", "ent0", "blk1", "ent1"))
        cnt, nb = int(exp["n"][i]), int(exp["blocks"][i])
        n["range_out"] += st == RANGE_OUT
        if st == RANGE_OUT or b0 == NONE:
            continue
        n["lower_gt_upper"] += bool(lk and uk and lo > up and cnt == 0)
        n["begin_differs"] += bool(lk) and (b0, e0) != (int(other["blk0"][i]), int(other["ent0"][i]))
        if lk:
            land = gc.seek_to_key_inner(s, lo, mvcc)
            p = bisect.bisect_left(s.first_keys, lo) if mvcc else bisect.bisect_right(s.first_keys, lo)
            n["begin_spill"] += lk == INCLUDED and land == (max(p - 1, 0) + 1, 0)
            n["excl_cross"] += lk == EXCLUDED and land[0] < len(s.blocks) and s.blocks[land[0]][land[1]][0] == lo \
                and b0 != land[0]
        size = lambda b: s.ends[b] - 4 - s.metas[b][0]
        if cnt:
            n["end_ent0"] += e1 == 0 and b1 < len(s.blocks)
            n["end_sst_end"] += b1 == len(s.blocks)
            n["one_block"] += nb == 1 and b1 == b0
            n["ge65_blocks"] += nb >= 65
            last = b1 if e1 else b1 - 1
            n["big_first"] += size(b0) > kGetLdsBlock and last > b0
            n["big_last"] += size(last) > kGetLdsBlock and last > b0
        if uk:  # blocks with distinct first keys whose images equal the upper bound's: whole keys decide
            ties = [j for j, fk in enumerate(s.first_keys) if gc.image(fk) == gc.image(up)]
            n["end_image_tie"] += len({s.first_keys[j] for j in ties}) >= 3 and ties[0] < b1 < ties[-1]
    return {k: int(v) for k, v in n.items()}


# ------------------------------------------------------------------------------ degenerate inputs
def corrupt_footer(buf):
    """The file with its bloom_offset pointing past the file: the open fails (MALFORMED)."""
    b = bytearray(buf)
    b[-4:] = (len(b) + 100).to_bytes(4, "big")
    return bytes(b)
