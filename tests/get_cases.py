"""SST sets and point lookups that reach chosen paths of lsmblk_get.hip -- TEST INFRASTRUCTURE.

The method of path_cases.py / sst_cases.py for the batched point read (lsmblk_sst_open_batch,
lsmblk_sst_get_batch); shared by test_get_cases.py (CPU: the generators reach what they were built
for) and test_gpu_get.py (GPU: every result field against the expectation).

  files         pyref.sst_file; what open must find comes from pyref.sst_open
  expectations  SsTableIterator::seek_to_key_inner, the move_to_key walk and the MVCC rule restated
                below over pyref.block_entries; the filters are pyref.Bloom.may_contain over
                pyref.fingerprint32 and key_within
  constants     kGetLdsBlock read out of the kernel source; IMG_BYTES is the index record's image
"""
import bisect
import os
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import path_cases as pc
from oracle import pyref

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsm_amd", "csrc", "lsmblk_get.hip")
kGetLdsBlock = pc.read_constants(_SRC, ("kGetLdsBlock",))["kGetLdsBlock"]
IMG_BYTES = 16  # lsmblk_sst_index.img_hi / img_lo (include/lsmblk.h)

ABSENT, FOUND, TOMBSTONE, RANGE_OUT, BLOOM_OUT = 0, 1, 2, 3, 4
NONE = 0xFFFFFFFF
FIELDS = ("status", "blk", "ent", "hit_blk", "hit_ent", "vlen", "ts", "val_pos")
MODES = ((False, False), (True, False), (False, True), (True, True))  # (no_filter, mvcc)


@dataclass
class Sst:
    buf: bytes
    bs: int
    entries: list
    metas: list = field(default_factory=list)      # pyref.sst_open: (offset, first_key, last_key)
    max_ts: int = 0
    bloom: object = None
    meta_offset: int = 0
    blocks: list = field(default_factory=list)     # per block [(key, ts, value, value offset in the file)]
    first_keys: list = field(default_factory=list)

    @property
    def ends(self):
        return [m[0] for m in self.metas[1:]] + [self.meta_offset]


def make_sst(entries, bs):
    buf = pyref.sst_file(entries, bs)
    metas, max_ts, bloom, meta_offset = pyref.sst_open(buf)
    s = Sst(buf, bs, entries, metas, max_ts, bloom, meta_offset)
    for (off, _, _), end in zip(metas, s.ends):
        blk = buf[off:end - 4]
        data, offsets = pyref.block_decode(blk)
        ents = pyref.block_entries(blk)
        s.blocks.append([(k, ts, v, off + o + 14 + int.from_bytes(data[o + 2:o + 4], "big"))
                         for (k, ts, v), o in zip(ents, offsets)])
    s.first_keys = [m[1] for m in metas]
    return s


# ------------------------------------------------------------------------------ the read, restated
def block_seek(ents, key):
    """BlockIterator::seek_to_key (src/block/iterator.rs:80-94): stops at the first equal probe."""
    lo, hi = 0, len(ents)
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if ents[mid][0] < key:
            lo = mid + 1
        elif ents[mid][0] > key:
            hi = mid
        else:
            return mid
    return lo


def seek_to_key_inner(s, key, mvcc):
    """SsTableIterator::seek_to_key_inner (src/table/iterator.rs:56-68) -> (blk, ent); blk == the
    block count: the iterator is invalid.  mvcc: the first entry in SST order with key >= the query."""
    p = bisect.bisect_left(s.first_keys, key) if mvcc else bisect.bisect_right(s.first_keys, key)
    b = max(p - 1, 0)  # find_block_idx, src/table.rs:253-257
    ents = s.blocks[b]
    e = bisect.bisect_left([x[0] for x in ents], key) if mvcc else block_seek(ents, key)
    if e == len(ents):  # the spill
        b, e = b + 1, 0
    return b, e


def lookup(s, key, read_ts, no_filter, mvcc, fp=pyref.fingerprint32):
    """One lookup -> the result record's fields (val_pos relative to the file)."""
    miss = dict(blk=NONE, ent=NONE, hit_blk=NONE, hit_ent=NONE, vlen=0, ts=0, val_pos=None, value=None)
    if not no_filter:
        if not (s.first_keys[0] <= key <= s.metas[-1][2]):  # key_within, src/lsm_storage.rs:136-138
            return dict(miss, status=RANGE_OUT)
        if not s.bloom.may_contain(fp(key)):
            return dict(miss, status=BLOOM_OUT)
    b, e = seek_to_key_inner(s, key, mvcc)
    out = dict(miss, status=ABSENT, blk=b, ent=e)
    while b < len(s.blocks):  # move_to_key / SsTableIterator::next: forward while the key's versions are too new
        k, ts, v, vpos = s.blocks[b][e]
        if k != key:
            break
        if ts <= read_ts:
            return dict(out, status=FOUND if v else TOMBSTONE, hit_blk=b, hit_ent=e, vlen=len(v), ts=ts, val_pos=vpos,
                        value=v if v else None)
        e += 1
        if e == len(s.blocks[b]):
            b, e = b + 1, 0
    return out


# ------------------------------------------------------------------------------ generators
def gen_entries(seed, nkeys=600, alphabet=b"abcd", maxver=6, tomb=0.25, klen=(1, 9), vlen=(1, 40), prefix=b""):
    rng = np.random.default_rng(seed)
    keys = set()
    while len(keys) < nkeys:
        keys.add(prefix + bytes(rng.choice(list(alphabet), int(rng.integers(*klen))).astype(np.uint8)))
    out = []
    for k in sorted(keys):
        tss = sorted({int(t) for t in rng.integers(1, 1000, int(rng.integers(1, maxver + 1)))}, reverse=True)
        for ts in tss:
            v = b"" if rng.random() < tomb else bytes(rng.integers(0, 256, int(rng.integers(*vlen)), dtype=np.uint8))
            out.append((k, ts, v))
    return out


def gen_queries(s, rng, extra=()):
    keys = sorted({k for k, _, _ in s.entries})
    qs = list(keys) + [k[:-1] for k in keys if len(k) > 1] + [k + bytes([int(rng.integers(97, 102))]) for k in keys]
    qs += [b"A", b"\x00", b"e", b"zz", keys[-1] + b"\xff", keys[0][:1]] + list(extra)
    tss = sorted({ts for _, ts, _ in s.entries})
    read_ts = [int(rng.choice([0, tss[0], int(rng.choice(tss)), int(rng.choice(tss)), tss[-1], 1 << 60])) for _ in qs]
    return qs, read_ts


def threshold_entries():
    """One SST at block_size 4096 whose blocks lie on both sides of kGetLdsBlock: single-entry blocks
    of exactly kGetLdsBlock and kGetLdsBlock + 1 bytes (18 + key + value bytes), a far larger one,
    and a key whose versions run from an ordinary block through an oversized one."""
    big = lambda k, ts, size: (k, ts, bytes((len(k) + i) & 0xFF for i in range(size - 18 - len(k))))
    ents = [(b"a%03d" % i, 7, b"v%d" % i) for i in range(40)]
    ents += [big(b"b-at", 9, kGetLdsBlock), (b"b-at", 5, b"older"), big(b"c-over", 9, kGetLdsBlock + 1), (b"c-over", 5, b"")]
    ents += [big(b"d-huge", 9, 3 * kGetLdsBlock), (b"d-huge", 3, b"tail")]
    ents += [(b"e-run", 50, b"new"), big(b"e-run", 40, kGetLdsBlock + 700), (b"e-run", 30, b"old"), (b"f", 1, b"last")]
    return ents


@dataclass
class Case:
    name: str
    ssts: list
    q_sst: list
    keys: list
    read_ts: list

    @property
    def files(self):
        return b"".join(s.buf for s in self.ssts)

    @property
    def file_off(self):
        return [0] + list(np.cumsum([len(s.buf) for s in self.ssts]))


def _case(name, ssts, seed, extra=()):
    rng = np.random.default_rng(seed)
    q_sst, keys, read_ts = [], [], []
    for i, s in enumerate(ssts):
        qs, ts = gen_queries(s, rng, extra)
        q_sst += [i] * len(qs)
        keys += qs
        read_ts += ts
    return Case(name, ssts, q_sst, keys, read_ts)


TIE_PREFIX = b"shared-prefix-of-20B"  # longer than the image: every first-key image of that SST is equal
CASES = ("bs128", "bs256", "bs4096", "ties", "threshold")


@lru_cache(maxsize=None)
def case(name):
    if name == "bs128":
        return _case(name, [make_sst(gen_entries(11), 128), make_sst(gen_entries(12), 128)], 1)
    if name == "bs256":
        # the third SST: one version per key, so its filter has 10 bits per distinct key (~1 % false positives)
        return _case(name, [make_sst(gen_entries(21), 256), make_sst(gen_entries(22), 256),
                            make_sst(gen_entries(23, maxver=1), 256)], 2)
    if name == "bs4096":
        return _case(name, [make_sst(gen_entries(31, vlen=(1, 200)), 4096), make_sst(gen_entries(32, nkeys=900), 4096)], 3)
    if name == "ties":
        tie = make_sst(gen_entries(41, nkeys=300, prefix=TIE_PREFIX), 128)
        part = make_sst(gen_entries(42, nkeys=200, prefix=TIE_PREFIX[:IMG_BYTES - 2], klen=(1, 6)), 128)
        return _case(name, [tie, make_sst(gen_entries(43, nkeys=200), 256), part], 4,
                     extra=(TIE_PREFIX, TIE_PREFIX[:IMG_BYTES], TIE_PREFIX[:IMG_BYTES] + b"\x00", TIE_PREFIX + b"zzzz"))
    if name == "threshold":
        s = make_sst(threshold_entries(), 4096)
        c = _case(name, [s, make_sst(gen_entries(51, nkeys=100), 4096)], 5)
        for k in (b"b-at", b"c-over", b"d-huge", b"e-run"):  # every version boundary of the large entries
            for ts in (0, 2, 3, 4, 5, 8, 9, 29, 30, 39, 40, 49, 50, 99):
                c.q_sst.append(0)
                c.keys.append(k)
                c.read_ts.append(ts)
        return c
    raise KeyError(name)


@lru_cache(maxsize=None)
def expected(name, no_filter, mvcc):
    """Every lookup of the case -> ({field: numpy array}, values list, val_off); val_pos absolute."""
    c = case(name)
    fpc = {}
    fp = lambda k: fpc[k] if k in fpc else fpc.setdefault(k, pyref.fingerprint32(k))
    rows = [lookup(c.ssts[s], k, ts, no_filter, mvcc, fp) for s, k, ts in zip(c.q_sst, c.keys, c.read_ts)]
    fo = c.file_off
    out = {f: np.array([r[f] for r in rows], np.uint64) for f in FIELDS if f != "val_pos"}
    out["val_pos"] = np.array([0 if r["val_pos"] is None else fo[s] + r["val_pos"] for r, s in zip(rows, c.q_sst)], np.uint64)
    values = [r["value"] for r in rows]
    val_off = np.concatenate([[0], np.cumsum([len(v) if v else 0 for v in values])]).astype(np.uint32)
    return out, values, val_off


# ------------------------------------------------------------------------------ coverage classifiers
def image(key):
    return key[:IMG_BYTES].ljust(IMG_BYTES, b"\0")


def classes(name):
    """Counts of the input classes the case reaches (per case, over all its SSTs and lookups)."""
    c = case(name)
    n = dict(dup_first=0, land_not_first=0, modes_differ=0, mvcc_cross=0, spill=0, end_invalid=0, found=0, tombstone=0,
             invisible=0, bloom_out=0, bloom_false_pos=0, range_out=0, image_tie=0, big_block=0, big_walk=0, at_lds=0)
    for s in c.ssts:
        n["dup_first"] += sum(a == b for a, b in zip(s.first_keys, s.first_keys[1:]))
        sizes = [end - 4 - off for (off, _, _), end in zip(s.metas, s.ends)]
        n["big_block"] += sum(z > kGetLdsBlock for z in sizes)
        n["at_lds"] += sum(z == kGetLdsBlock for z in sizes)
    ref, _, _ = expected(name, False, False)
    nof, _, _ = expected(name, True, False)
    mv, _, _ = expected(name, False, True)
    nmv, _, _ = expected(name, True, True)
    for i, (si, k) in enumerate(zip(c.q_sst, c.keys)):
        s = c.ssts[si]
        present = any(k == e[0] for e in s.blocks[min(int(nmv["blk"][i]), len(s.blocks) - 1)]) and nmv["blk"][i] < len(s.blocks)
        if nof["blk"][i] < len(s.blocks) and present:
            b, e = int(nof["blk"][i]), int(nof["ent"][i])
            if s.blocks[b][e][0] == k and (b, e) != (int(nmv["blk"][i]), int(nmv["ent"][i])):
                n["land_not_first"] += 1
        n["modes_differ"] += any(ref[f][i] != mv[f][i] for f in FIELDS)
        n["mvcc_cross"] += nmv["status"][i] in (FOUND, TOMBSTONE) and nmv["hit_blk"][i] != nmv["blk"][i]
        p = bisect.bisect_right(s.first_keys, k)
        n["spill"] += nof["blk"][i] == max(p - 1, 0) + 1 and nof["ent"][i] == 0
        n["end_invalid"] += nof["blk"][i] == len(s.blocks)
        n["found"] += ref["status"][i] == FOUND
        n["tombstone"] += ref["status"][i] == TOMBSTONE
        n["invisible"] += nof["status"][i] == ABSENT and nof["blk"][i] < len(s.blocks) and \
            s.blocks[int(nof["blk"][i])][int(nof["ent"][i])][0] == k
        n["bloom_out"] += ref["status"][i] == BLOOM_OUT
        n["range_out"] += ref["status"][i] == RANGE_OUT
        absent = all(k != e[0] for e in s.entries)
        n["bloom_false_pos"] += absent and ref["status"][i] not in (BLOOM_OUT, RANGE_OUT)
        # blocks with DISTINCT first keys whose images equal the query's: whole keys must decide
        ties = [j for j, fk in enumerate(s.first_keys) if image(fk) == image(k)]
        n["image_tie"] += len({s.first_keys[j] for j in ties}) >= 3 and ties[0] < int(nof["blk"][i]) < ties[-1]
        hb = int(nmv["hit_blk"][i])
        if hb != NONE:
            off, end = s.metas[hb][0], s.ends[hb]
            n["big_walk"] += end - 4 - off > kGetLdsBlock and hb != nmv["blk"][i]
    return {k: int(v) for k, v in n.items()}
