"""Inputs that put SSTs on chosen paths of the container kernels -- TEST INFRASTRUCTURE.

The method of path_cases.py, for lsmblk_sst.hip (layout, data, meta, bloom, seek) and the meta_*
kernels of lsmblk_gpu.hip; shared by test_sst_cases.py (CPU) and test_gpu_sst_paths.py (GPU):

  constants    kBloomLds, kCrcSeg, kCrcChunk, kCrcPad, kMetaTile, kMetaImg read out of the kernel
               sources; every probe below is derived from them
  classifiers  numpy restatements of the predicates that pick a path (fingerprint32's length
               classes, the bloom kernel's LDS switch and CRC chunking, meta_write_kernel's tile
               image).  They only ASSERT COVERAGE; expected bytes come from oracle/ alone.
  generators   streams of SSTs (one segment of the KV stream each) and seek probes.

A generator returns a Case; the check_* functions take the constants they check against, so a
case built for other constants fails them.
"""
import os
from dataclasses import dataclass, field

import numpy as np

import path_cases as pc
from oracle import oracle as O
from oracle import pyref

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsm_amd", "csrc")
SOURCES = {"kBloomLds": "lsmblk_sst.hip", "kCrcSeg": "lsmblk_dev.hpp", "kCrcChunk": "lsmblk_dev.hpp",
           "kCrcPad": "lsmblk_dev.hpp", "kMetaTile": "lsmblk_gpu.hip", "kMetaImg": "lsmblk_gpu.hip"}


@dataclass(frozen=True)
class Consts:
    kBloomLds: int
    kCrcSeg: int
    kCrcChunk: int
    kCrcPad: int
    kMetaTile: int
    kMetaImg: int

    @property
    def lds_chunk(self):
        """crc_lds's chunk: 64 whole lane windows."""
        return 64 * self.kCrcSeg


def kernel_constants(path=None):
    """The container kernels' constants.  path: {constant: source file} for those to be read from
    another file than lsm_amd/csrc's (a retuned scratch copy); a missing constant raises."""
    path = path or {}
    out = {}
    for name, src in SOURCES.items():
        out.update(pc.read_constants(path.get(name, os.path.join(_CSRC, src)), (name,)))
    return Consts(**out)


C = kernel_constants()
# sst_layout_kernel scans the file sizes in rounds of its 1024 threads (`r += kWgScan`, the
# workgroup scan's width in lsmblk_dev.hpp, tied to 16 waves by a static_assert there) and carries
# the running total from round to round (block_round1024)
LAYOUT_ROUND = 1024
LAYOUT_NSST = (1, LAYOUT_ROUND - 1, LAYOUT_ROUND, LAYOUT_ROUND + 1, 2 * LAYOUT_ROUND, 2 * LAYOUT_ROUND + 1,
               2 * LAYOUT_ROUND + 452)  # the last: a third round partly filled (2500 today)


# ------------------------------------------------------------------------------- streams of SSTs
@dataclass
class Case:
    kv: O.KV
    ent: np.ndarray   # u32[nsst + 1]: SST s = entries [ent[s], ent[s + 1]) (the encode's segments)
    bs: int
    tag: list = field(default_factory=list)   # per SST, what it is there for


def build(specs, bs, seed, tags=None):
    """specs: per SST (key lengths, value lengths).  Keys are [entry index BE u24][random ...]
    (sorted and unique where every key has >= 4 bytes), values random."""
    rng = np.random.default_rng(seed)
    klen = np.concatenate([np.asarray(k, np.int64) for k, _ in specs])
    vlen = np.concatenate([np.asarray(v, np.int64) for _, v in specs])
    assert len(klen) == len(vlen) < 1 << 24
    kv = pc._kv(klen, vlen, pc._be(np.arange(len(klen)), 3), 3, rng)
    ent = np.concatenate([[0], np.cumsum([len(k) for k, _ in specs])]).astype(np.uint32)
    return Case(kv, ent, bs, list(tags) if tags is not None else [None] * len(specs))


def entries_of(case, s=None):
    """The (key, ts, value) tuples of SST s (None: of the whole stream), for pyref."""
    kv = case.kv
    lo, hi = (0, kv.n) if s is None else (int(case.ent[s]), int(case.ent[s + 1]))
    kb, vb = kv.keys.tobytes(), kv.vals.tobytes()
    ko, vo, ts = kv.key_off.tolist(), kv.val_off.tolist(), kv.ts.tolist()
    return [(kb[ko[i]:ko[i + 1]], ts[i], vb[vo[i]:vo[i + 1]]) for i in range(lo, hi)]


def expected_files(case):
    """pyref.sst_file of every SST."""
    ents = entries_of(case)
    return [pyref.sst_file(ents[int(a):int(b)], case.bs) for a, b in zip(case.ent[:-1], case.ent[1:])]


def bloom_len(n):
    """nbytes + 1 of an n-key filter: build_from_key_hashes's size (bloom.rs:80-88) plus k."""
    return (max(n * pyref.Bloom.bloom_bits_per_key(n, 0.01), 64) + 7) // 8 + 1


@dataclass
class Layout:
    """The oracle's blocks of a case and the sections' sizes per SST (sizes follow from the key
    and value lengths alone)."""
    blocks: np.ndarray
    blk_off: np.ndarray
    sst_blk: np.ndarray    # u32[nsst + 1]
    data_len: np.ndarray   # blocks + 4 B CRC each (= meta_offset)
    meta_len: np.ndarray
    bloom_len: np.ndarray  # nbytes + 1
    bloom_off: np.ndarray  # data + meta + 4 (= bloom_offset)
    file_len: np.ndarray
    file_off: np.ndarray   # nsst + 1
    rec: np.ndarray        # per block: its BlockMeta record, 24 + first key + last key


def layout(case):
    kv, ent = case.kv, case.ent.astype(np.int64)
    rc, blocks, off = O.encode_segments(kv, case.ent, case.bs)
    assert rc == 0
    off = off.astype(np.int64)
    cnt = pc.block_entry_counts(blocks, off) if len(off) > 1 else np.zeros(0, np.int64)
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    assert first[-1] == kv.n
    sst_blk = np.searchsorted(first, ent).astype(np.int64)
    assert (first[sst_blk] == ent).all(), "an SST does not start a block"
    kl = np.diff(kv.key_off.astype(np.int64))
    rec = 24 + kl[first[:-1]] + kl[first[1:] - 1]
    rsum = np.concatenate([[0], np.cumsum(rec)])
    nb = np.diff(sst_blk)
    data_len = off[sst_blk[1:]] - off[sst_blk[:-1]] + 4 * nb
    meta_len = 16 + rsum[sst_blk[1:]] - rsum[sst_blk[:-1]]
    bl = np.array([bloom_len(int(n)) for n in np.diff(ent)], np.int64)
    bloom_off = data_len + meta_len + 4
    file_len = bloom_off + bl + 4 + 4
    return Layout(blocks, off.astype(np.uint64), sst_blk.astype(np.uint32), data_len, meta_len, bl, bloom_off,
                  file_len, np.concatenate([[0], np.cumsum(file_len)]), rec)


def section_of(lay, s, byte):
    """The section of SST s that holds byte `byte` of its file."""
    return "data" if byte < lay.data_len[s] else ("meta" if byte < lay.bloom_off[s] else "bloom")


def steer(specs, bs, seed, fillers, quantity, targets, tags=None):
    """Lengthen the one-entry filler SSTs `fillers` (indices into specs) by 0..3 value bytes so
    that quantity(layout, s + 1) & 3 == target for the SST after each -- a file's length grows by
    one per value byte and nothing else moves."""
    specs = [(np.array(k), np.array(v)) for k, v in specs]
    lay = layout(build(specs, bs, seed))
    shift = 0
    for f, t in zip(fillers, targets):
        add = (t - int(quantity(lay, f + 1)) - shift) & 3
        specs[f][1][0] += add
        shift += add
    return build(specs, bs, seed, tags)


def bloom_addr(lay, s):
    return lay.file_off[s] + lay.bloom_off[s]


# ------------------------------------------------------------------------------- 1. fingerprint32
FP_CLASSES = ("<=4", "5-12", "13-24", ">24")
FP_LONG = (200, 255, 256, 300, 1000)
FP_LAST = (3, 11, 23, 127)   # the stream's last key, one length per class


def fp_class(n):
    n = np.asarray(n)
    return np.where(n <= 4, 0, np.where(n <= 12, 1, np.where(n <= 24, 2, 3)))


def fp_iters(n):
    """The > 24 branch's loop count."""
    return (np.asarray(n) - 1) // 20


def fingerprint_stream(seed=401):
    """One-entry SSTs at block_size 16 (one key per 64-bit filter): key lengths 1..130, the same
    again with every byte >= 0x80, then FP_LONG; value lengths cycle 0..15, a step further every
    16 keys, so that the block lengths (18 + key + value) take every residue mod 16."""
    lens = list(range(1, 131)) * 2 + list(FP_LONG)
    case = build([([k], [(i + i // 16) % 16]) for i, k in enumerate(lens)], 16, seed, tags=lens)
    kv = case.kv
    kv.keys[int(kv.key_off[130]):int(kv.key_off[260])] |= 0x80
    return case


def reorder_last(case, last):
    """The same SSTs with SST `last` moved to the end of the stream."""
    kv = case.kv
    perm = np.array([i for i in range(kv.n) if i != last] + [last])
    return Case(O.gather(kv, perm), case.ent, case.bs, [case.tag[i] for i in perm]), perm


def fp_last_indices(case):
    """For each length class, the SST (of the high-byte set where there is one) of FP_LAST's length."""
    return [max(i for i, k in enumerate(case.tag[:260]) if k == want) for want in FP_LAST]


def check_fingerprint_stream(case):
    lens = np.asarray(case.tag)
    kv = case.kv
    assert (np.diff(case.ent.astype(np.int64)) == 1).all() and case.bs == 16
    assert (np.diff(kv.key_off.astype(np.int64)) == lens).all()
    have = set(lens.tolist())
    for lo in (4, 12, 24):                       # class bounds, both sides
        assert {lo, lo + 1} <= have and fp_class(lo) != fp_class(lo + 1)
    for lo in (40, 60, 80, 100, 120):            # steps of the loop count
        assert {lo, lo + 1} <= have and fp_iters(lo + 1) == fp_iters(lo) + 1
    assert set(range(1, 131)) | set(FP_LONG) <= have
    hi = kv.keys[int(kv.key_off[130]):int(kv.key_off[260])]
    assert (hi >= 0x80).all() and sorted(lens[130:260].tolist()) == list(range(1, 131))
    assert set(np.diff(kv.val_off.astype(np.int64)).tolist()) == set(range(16))
    assert set((np.diff(layout(case).blk_off.astype(np.int64)) % 16).tolist()) == set(range(16))
    assert [int(fp_class(lens[i])) for i in fp_last_indices(case)] == [0, 1, 2, 3]


# ------------------------------------------------------------------------------- 2. bloom sizes
def count_for(length, lo_only=False):
    """The smallest key count whose bloom_len is `length`, or None (ceil(1.25 n) skips lengths)."""
    g = max(1, (length - 1) * 8 // 10)
    for n in range(max(1, g - 3), g + 4):
        if bloom_len(n) == length:
            return n
    return None


def edge_counts(mult):
    """Key counts that put bloom_len on `mult`, on the nearest reachable length under it and on
    the nearest over it."""
    out = []
    for rng_ in (range(mult - 1, mult - 4, -1), (mult,), range(mult + 1, mult + 4)):
        n = next((count_for(L) for L in rng_ if count_for(L) is not None), None)
        if n is not None:
            out.append(n)
    return out


def bloom_counts(c=C):
    """{group: key counts}: "min" (the 64-bit floor and the first sizes over it), "lds" (crc_lds
    chunk edges for 1, 2, 3 chunks and the largest LDS filter), "global" (the smallest global
    filter and the chunk edges of the first two kCrcChunk multiples over the switch)."""
    lds = [n for m in (1, 2, 3) for n in edge_counts(m * c.lds_chunk)] + [count_for(c.kBloomLds)]
    m0 = c.kBloomLds // c.kCrcChunk + 1
    glob = [count_for(c.kBloomLds + 1)] + [n for m in (m0, m0 + 1) for n in edge_counts(m * c.kCrcChunk)]
    assert None not in lds and None not in glob, "the LDS switch is not reachable by a key count"
    return {"min": [1, 6, 7, 8], "lds": lds, "global": glob}


def max_lds_count(c=C):
    """The largest key count whose filter is still built in LDS."""
    n = c.kBloomLds * 8 // 10 + 8
    while bloom_len(n) > c.kBloomLds:
        n -= 1
    return n


def bloom_path(n, c=C):
    """(path, CRC chunks) of an n-key filter: sst_bloom_kernel's `lds` and the fold loops."""
    L = bloom_len(n)
    if L <= c.kBloomLds:
        return "lds", -(-L // c.lds_chunk)
    return "global", -(-L // c.kCrcChunk)


def _bloom_spec(n, rng):
    return rng.integers(8, 41, n), np.zeros(n, np.int64)


def bloom_stream(group, c=C, seed=402):
    """The SSTs of one group at block_size 4096: sorted unique keys of 8-40 bytes, empty values.
    "global": before each a one-entry filler that steers (file_off + bloom_offset) & 3 through
    0, 1, 2, 3, ...; "lds-a" / "lds-b" split the LDS group (Python cost of the expectation)."""
    rng = np.random.default_rng(seed)
    counts = bloom_counts(c)
    if group != "global":
        ns = {"min": counts["min"], "lds-a": counts["lds"][:len(counts["lds"]) // 2],
              "lds-b": counts["lds"][len(counts["lds"]) // 2:]}[group]
        return build([_bloom_spec(n, rng) for n in ns], 4096, seed, tags=ns)
    specs, tags = [], []
    for n in counts["global"]:
        specs += [([5], [0]), _bloom_spec(n, rng)]
        tags += [0, n]
    fillers = list(range(0, len(specs), 2))
    return steer(specs, 4096, seed, fillers, bloom_addr, [i & 3 for i in range(len(fillers))], tags)


def check_bloom_counts(counts, c=C):
    """The key counts sit where they were meant to, for the constants c."""
    W, K = c.lds_chunk, c.kCrcChunk
    L = {g: [bloom_len(n) for n in ns] for g, ns in counts.items()}
    assert L["min"][:2] == [9, 9] and L["min"][2] > 9 and L["min"][3] > L["min"][2]
    assert c.kBloomLds in L["lds"] and c.kBloomLds + 1 in L["global"], "the LDS switch"
    assert all(bloom_path(n, c)[0] == "lds" for n in counts["lds"] + counts["min"])
    assert all(bloom_path(n, c)[0] == "global" for n in counts["global"])
    for m in (1, 2, 3):
        near = [x - m * W for x in L["lds"] if abs(x - m * W) <= 3]
        assert near and min(near) < 0 < max(near), f"crc_lds chunk edge {m * W}: {near}"
    assert max(bloom_path(n, c)[1] for n in counts["lds"]) >= 3, "no LDS filter of three chunks"
    m0 = c.kBloomLds // K + 1
    for m in (m0, m0 + 1):
        near = [x - m * K for x in L["global"] if abs(x - m * K) <= 3]
        assert near and min(near) < 0 < max(near) and 0 in near, f"global chunk edge {m * K}: {near}"


def check_bloom_global(case, lay, files_addr=0, c=C):
    """Every non-filler SST is on the global path and the bloom addresses' low two bits take all
    four values."""
    big = [s for s, n in enumerate(case.tag) if n]
    assert big and all(bloom_path(case.tag[s], c)[0] == "global" for s in big)
    assert all(int(case.ent[s + 1] - case.ent[s]) == 1 for s, n in enumerate(case.tag) if not n)
    dsh = sorted({int(files_addr + bloom_addr(lay, s)) & 3 for s in big})
    assert dsh == [0, 1, 2, 3], dsh
    return dsh


# ------------------------------------------------------------------------------- 3. layout
def layout_stream(seed=403, nsst=max(LAYOUT_NSST)):
    """One-entry and two-entry SSTs at block_size 16 (every entry its own block)."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(1, 3, nsst)
    return build([(rng.integers(4, 13, n), rng.integers(0, 21, n)) for n in cnt], 16, seed)


def capacity_stream(which, c=C, seed=409):
    """Section 3's stream of LAYOUT_ROUND + 1 SSTs ("layout") or the smallest global-path SST
    ("global"), after a one-entry filler SST that leaves the next file at 1 mod 4."""
    rng = np.random.default_rng(seed)
    if which == "layout":
        body = [(rng.integers(4, 13, n), rng.integers(0, 21, n)) for n in rng.integers(1, 3, LAYOUT_ROUND + 1)]
        bs = 16
    else:
        body, bs = [_bloom_spec(count_for(c.kBloomLds + 1), rng)], 4096
    return steer([([5], [0])] + body, bs, seed, [0], lambda lay, s: lay.file_off[s], [1])


def prefix(case, lay, nsst):
    """(entries, blocks) of the first nsst SSTs."""
    return int(case.ent[nsst]), int(lay.sst_blk[nsst])


def check_layout_stream(case, lay):
    assert len(case.ent) - 1 == max(LAYOUT_NSST) > 2 * LAYOUT_ROUND
    assert {LAYOUT_ROUND - 1, LAYOUT_ROUND, LAYOUT_ROUND + 1, 2 * LAYOUT_ROUND, 2 * LAYOUT_ROUND + 1} < set(LAYOUT_NSST)
    assert set(np.diff(case.ent.astype(np.int64)).tolist()) == {1, 2}
    assert (np.diff(lay.sst_blk.astype(np.int64)) == np.diff(case.ent.astype(np.int64))).all()
    assert len(set(lay.file_len.tolist())) > 16


# ------------------------------------------------------------------------------- 4. BlockMeta tiles
# Records of one-entry blocks are even (24 + 2 x key length), so a tile of odd size needs a block
# of two entries with keys of k and k + 1 bytes; block_size 16 holds one entry only.  At META_BS an
# entry with a META_BS-byte value is always alone in its block and two value-less ones share one.
META_BS = 256


@dataclass
class Tiles:
    """meta_write_kernel's per-tile quantities, restated: t_lo, t_hi (section bytes of the tile's
    first record and the end of its last), lead = low 4 address bits of the first record, and
    lhs = lead + (t_hi - t_lo), the left-hand side of `<= kMetaImg`."""
    t_lo: np.ndarray
    t_hi: np.ndarray
    lead: np.ndarray
    lhs: np.ndarray

    def lds(self, c=C):
        return self.lhs <= c.kMetaImg


def meta_tiles(rec, seg_blk, meta_addr=0, c=C):
    rec, seg_blk = np.asarray(rec, np.int64), np.asarray(seg_blk, np.int64)
    nblk = len(rec)
    pos = np.concatenate([[0], np.cumsum(rec)])
    seg = np.searchsorted(seg_blk[:-1], np.arange(nblk), side="right") - 1  # largest s: seg_blk[s] <= b
    dst = pos[:-1] + 16 * seg + 4
    b0 = np.arange(0, nblk, c.kMetaTile)
    b1 = np.minimum(b0 + c.kMetaTile, nblk) - 1
    t_lo, t_hi = dst[b0], dst[b1] + rec[b1]
    lead = (meta_addr + t_lo) & 15
    return Tiles(t_lo, t_hi, lead, lead + t_hi - t_lo)


def _meta_segments(c, ntile, empty_segments):
    """seg_blk of the tile stream: SSTs of kMetaTile - 1, kMetaTile and kMetaTile + 1 blocks (the
    third ends on a tile edge), boundaries one block after and one before an edge, a run of empty
    segments inside tile 7, and a few long SSTs."""
    T = c.kMetaTile
    cuts = [0, T - 1, 2 * T - 1, 3 * T, 4 * T + 1, 6 * T - 1]
    cuts += [7 * T + T // 2] * (4 if empty_segments else 1)
    cuts += [16 * T, 32 * T + T // 2, ntile * T + 1]
    return np.asarray(cuts, np.int64)


def meta_stream(meta_addr=0, c=C, seed=404, empty_segments=True):
    """Tiles of kMetaTile blocks at block_size META_BS, key lengths chosen per tile (a one-entry
    block's record is 24 + 2 x key length; a tile of odd size ends in a two-entry block with keys
    of k and k + 1 bytes) -> (Case, seg_blk).  In order:
      16 small tiles whose sizes are 0, 1, ..., 15 mod 16: their leads run through the triangular
              numbers, a permutation of 0..15, so the LDS side sees every lead and every size & 15
      17 tiles with lhs = kMetaImg - 8 .. kMetaImg + 8 (each one's lead is the lhs before it & 15)
      3 x 4 tiles: a small one that sets the lead, lhs = kMetaImg, a small one, lhs = kMetaImg + 1
      one last tile of a single block."""
    T, K = c.kMetaTile, c.kMetaImg
    small = T * (24 + 2 * 8)
    plan = [("size", small + e) for e in range(16)]                       # (what, value)
    plan += [("lhs", v) for v in range(K - 8, K + 9)]
    for L in (3, 7, 11):
        plan += [("next", L), ("lhs", K), ("next", L + 1), ("lhs", K + 1)]
    seg_blk = _meta_segments(c, len(plan), empty_segments)
    seg_of = lambda b: int(np.searchsorted(seg_blk[:-1], b, side="right")) - 1
    specs, lead = [], (meta_addr + 4) & 15
    for t, (what, v) in enumerate(plan):
        cross = 16 * (seg_of(t * T + T - 1) - seg_of(t * T))
        if what == "size":
            size = v
        elif what == "lhs":
            size = v - lead - cross
        else:  # the next tile's lead
            size = small + ((v - lead - small - cross) & 15)
        keys = size - 24 * T                     # first + last key bytes over the tile
        assert keys >= 8 * T
        k = pc._spread(keys // 2, T)
        for i in range(T):
            if i == T - 1 and keys & 1:
                specs.append(([k[i], k[i] + 1], [0, 0]))
            else:
                specs.append(([k[i]], [META_BS]))
        lead = (lead + size + cross) & 15
    specs.append(([9], [META_BS]))
    # the KV stream's segments are the non-empty SSTs; seg_blk keeps the empty ones
    case = build(specs, META_BS, seed)
    ent_of_blk = case.ent.astype(np.int64)      # one spec per block
    case.ent = ent_of_blk[np.unique(seg_blk)].astype(np.uint32)
    return case, seg_blk.astype(np.uint32)


def check_meta_stream(case, seg_blk, lay, meta_addr=0, c=C):
    T, K = c.kMetaTile, c.kMetaImg
    nblk = len(lay.rec)
    assert int(seg_blk[-1]) == nblk == len(lay.blk_off) - 1 and nblk >= 40 * T
    cnt = pc.block_entry_counts(lay.blocks, lay.blk_off.astype(np.int64))
    assert set(cnt.tolist()) == {1, 2}, "blocks of one and of two entries"
    t = meta_tiles(lay.rec, seg_blk, meta_addr, c)
    assert set(range(K - 8, K + 9)) <= set(t.lhs.tolist())
    for v in (K, K + 1):
        assert len(set(t.lead[t.lhs == v].tolist())) >= 4, (v, t.lead[t.lhs == v])
    lds = t.lds(c)
    assert set(t.lead[lds].tolist()) == set(range(16)), "leads on the LDS side"
    assert set(((t.t_hi - t.t_lo)[lds] & 15).tolist()) == set(range(16)), "span & 15 on the LDS side"
    sb = np.asarray(seg_blk, np.int64)
    edges = sb[1:-1] % T
    assert 0 in edges and 1 in edges and T - 1 in edges, "segment boundaries around a tile edge"
    assert {T - 1, T, T + 1} <= set(np.diff(sb).tolist()), "segment block counts"
    assert nblk % T == 1, "a last tile of one block"
    return t


def meta_coverage(name, t, c=C):
    lds = t.lds(c)
    return (f"{name}: {len(t.lhs)} tiles; lds {int(lds.sum())} (leads {sorted(set(t.lead[lds].tolist()))}, "
            f"lhs max {int(t.lhs[lds].max())}); direct {int((~lds).sum())} (leads "
            f"{sorted(set(t.lead[~lds].tolist()))}, lhs min {int(t.lhs[~lds].min())}); "
            f"kMetaImg on leads {sorted(t.lead[t.lhs == c.kMetaImg].tolist())}, +1 on "
            f"{sorted(t.lead[t.lhs == c.kMetaImg + 1].tolist())}")


def expected_metas(case, seg_blk):
    """pyref's BlockMeta section of every segment (an empty one: no records)."""
    ents = entries_of(case)
    out, s = [], 0
    for a, b in zip(seg_blk[:-1], seg_blk[1:]):
        if a == b:
            out.append(pyref.encode_block_meta([]))
            continue
        e0, e1 = int(case.ent[s]), int(case.ent[s + 1])
        out.append(pyref.encode_block_meta(pyref.sst_block_metas(ents[e0:e1], case.bs)))
        s += 1
    return out


# ------------------------------------------------------------------------------- 6. seek
@dataclass
class SeekCase:
    kv: O.KV
    seg: np.ndarray
    bs: int
    blocks: np.ndarray = None
    blk_off: np.ndarray = None
    q_blk: list = field(default_factory=list)
    q_key: list = field(default_factory=list)
    q_self: list = field(default_factory=list)   # the entry a probe must land on, or -1

    def encode(self):
        rc, self.blocks, self.blk_off = O.encode_segments(self.kv, self.seg, self.bs)
        assert rc == 0
        return self

    def block(self, b):
        return self.blocks[int(self.blk_off[b]):int(self.blk_off[b + 1])].tobytes()

    def block_keys(self, b):
        return [k for k, _, _ in pyref.block_entries(self.block(b))]

    def probe(self, b, key, want=-1):
        self.q_blk.append(b)
        self.q_key.append(bytes(key))
        self.q_self.append(want)

    def probe_whole_block(self, b):
        """For every entry: its key (lands on it), key + 0x00, key minus its last byte, and the
        key with its last byte one up and one down."""
        for i, k in enumerate(self.block_keys(b)):
            self.probe(b, k, i)
            self.probe(b, k + b"\x00")
            self.probe(b, k[:-1])
            if k[-1] < 255:
                self.probe(b, k[:-1] + bytes([k[-1] + 1]))
            if k[-1] > 0:
                self.probe(b, k[:-1] + bytes([k[-1] - 1]))

    def probe_ends(self, b):
        """The empty probe, 300 bytes of 0xFF, the block's first and last keys."""
        keys = self.block_keys(b)
        self.probe(b, b"")
        self.probe(b, b"\xff" * 300)
        self.probe(b, keys[0], 0)
        self.probe(b, keys[-1], len(keys) - 1)

    def expected(self):
        blk = {b: self.block(b) for b in set(self.q_blk)}
        return [O.seek_key(blk[b], k) for b, k in zip(self.q_blk, self.q_key)]

    def prefix_lens(self):
        """prefix_len of every entry of the probed blocks."""
        out = []
        for b in sorted(set(self.q_blk)):
            blk = self.block(b)
            n = int.from_bytes(blk[-2:], "big")
            out += [O.entry_verbatim(blk, i)[0] for i in range(n)]
        return np.asarray(out)


def _from_keys(keys, rng, vmax):
    keys = sorted(set(keys))
    ents = [(k, int(rng.integers(0, 1 << 40)), bytes(rng.integers(0, 256, int(rng.integers(0, vmax + 1)), dtype=np.uint8)))
            for k in keys]
    return O.KV.from_entries(ents)


def seek_prefix_case(bs, seed=405, n=700):
    """Keys = a 60-byte stem cut at a random length 20..60 plus a 1-5-byte tail, and at the end of
    the order a few keys that leave the stem at byte 0 and at byte 1 (prefix_len 0 and 1 inside a
    block that starts with a stem key).  Probes: whole blocks (first, middle, last), the ends of
    every block, and random cuts of keys."""
    rng = np.random.default_rng(seed)
    stem = bytes(rng.integers(16, 200, 60, dtype=np.uint8))
    keys = []
    for _ in range(n):
        # three tails in four start above every stem byte: the longer cut then sorts first, and a
        # block's entries share their own cut length with its first key
        tail = bytearray(rng.integers(0, 256, int(rng.integers(1, 6)), dtype=np.uint8))
        if rng.random() < 0.75:
            tail[0] = 200 + tail[0] % 56
        keys.append(stem[:int(rng.integers(20, 61))] + bytes(tail))
    keys += [bytes([stem[0] + 1 + i, 7, 7]) for i in range(3)] + [bytes([stem[0], stem[1] + 1 + i, 9]) for i in range(3)]
    kv = _from_keys(keys, rng, 30)
    c = SeekCase(kv, np.array([0, kv.n], np.uint32), bs).encode()
    nb = len(c.blk_off) - 1
    for b in sorted({0, nb // 2, nb - 1}):
        c.probe_whole_block(b)
    for b in range(nb):
        c.probe_ends(b)
    allk = [kv.entry(i)[0] for i in range(kv.n)]
    for _ in range(1500):
        k = allk[int(rng.integers(0, len(allk)))]
        c.probe(int(rng.integers(0, nb)), k[:int(rng.integers(0, len(k) + 1))] + (b"" if rng.random() < .5 else b"\x80"))
    return c


def seek_chain_case(bs, seed=406, depth=30, chains=6):
    """Chains k, k + a, k + a + b, ... `depth` deep: every key a strict prefix of the next."""
    rng = np.random.default_rng(seed)
    keys = []
    for ch in range(chains):
        k = bytes([20 + 30 * ch]) + bytes(rng.integers(0, 256, 2, dtype=np.uint8))
        for _ in range(depth):
            keys.append(k)
            k += bytes(rng.integers(0, 256, int(rng.integers(1, 4)), dtype=np.uint8))
    kv = _from_keys(keys, rng, 6)
    c = SeekCase(kv, np.array([0, kv.n], np.uint32), bs).encode()
    for b in range(len(c.blk_off) - 1):
        c.probe_whole_block(b)
        c.probe_ends(b)
    return c


def seek_big_case(seed=407, n=3200):
    """One block_size-65536 segment whose first block holds more than 2000 entries, and the block
    of the rest: every entry probed."""
    rng = np.random.default_rng(seed)
    keys = [i.to_bytes(2, "big") + bytes(rng.integers(0, 256, int(rng.integers(2, 10)), dtype=np.uint8)) for i in range(n)]
    kv = _from_keys(keys, rng, 8)
    c = SeekCase(kv, np.array([0, kv.n], np.uint32), 65536).encode()
    for b in range(len(c.blk_off) - 1):
        c.probe_whole_block(b)
        c.probe_ends(b)
    return c


def seek_tiny_case(seed=408):
    """One-entry and two-entry blocks (segments of one and two entries at block_size 4096)."""
    rng = np.random.default_rng(seed)
    keys = [bytes([i]) + bytes(rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8)) for i in range(1, 40)]
    kv = _from_keys(keys, rng, 10)
    seg = np.concatenate([[0], np.cumsum([1, 2] * 13)]).astype(np.uint32)
    c = SeekCase(kv, seg, 4096).encode()
    for b in range(len(c.blk_off) - 1):
        c.probe_whole_block(b)
        c.probe_ends(b)
    return c


def seek_coverage(name, c):
    p = c.prefix_lens()
    cnt = [int.from_bytes(c.block(b)[-2:], "big") for b in sorted(set(c.q_blk))]
    return (f"{name}: {len(c.q_key)} probes over {len(cnt)} blocks of {min(cnt)}..{max(cnt)} entries; "
            f"prefix_len {int(p.min())}..{int(p.max())}, {len(set(p.tolist()))} distinct")
