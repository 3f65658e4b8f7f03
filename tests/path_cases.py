"""Inputs that put blocks on chosen paths of the decode and emit kernels -- TEST INFRASTRUCTURE.

Three things live here, shared by test_path_cases.py (CPU) and test_gpu_paths.py (GPU):

  constants    kDecImg, kEmitKCap, ... read out of lsm_amd/csrc/lsmblk_gpu.hip, so that a probe
               follows a retuned constant instead of silently leaving the edge
  classifiers  plain numpy restatements of the predicates that choose a block's path (decode_block,
               dec_fast_outputs, emit_kernel's / fuse_emit's is_fast).  They only ASSERT COVERAGE:
               that a generated input really reaches the path or the side of a threshold it was
               built for.  Expected bytes always come from the oracle.
  generators   stream A (one entry per block, fast / big chosen per block), stream B (natural
               packing over five regimes) and the probe lists (one block per segment, on the
               thresholds), built as numpy arrays.

Every generator returns (kv, seg_start, block_size).
"""
import os
import re
from dataclasses import dataclass

import numpy as np

from lsm_amd import synth
from oracle import oracle as O

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsm_amd", "csrc", "lsmblk_gpu.hip")
_NAMES = ("kDecImg", "kDecMaxE", "kDecOut", "kEmitKCap", "kEmitICap", "kEmitMaxE", "kTile")


def read_constants(path, names):
    """{name: value} of `names`, from their `constexpr uint32_t NAME = N;` lines in `path` (N a
    decimal or hexadecimal literal, with or without the `u` suffix)."""
    with open(path) as f:
        text = f.read()
    out = {}
    for name in names:
        m = re.search(r"^constexpr\s+uint32_t\s+%s\s*=\s*(0[xX][0-9A-Fa-f]+|\d+)[uU]?\s*;" % name, text, re.M)
        if not m:
            raise RuntimeError(f"{name}: no `constexpr uint32_t {name} = N;` in {path}")
        out[name] = int(m.group(1), 0)
    return out


def kernel_constants(path=_SRC):
    """{name: value} of the dispatch constants of the decode and emit kernels."""
    return read_constants(path, _NAMES)


K = kernel_constants()
kDecImg, kDecMaxE, kDecOut = K["kDecImg"], K["kDecMaxE"], K["kDecOut"]
kEmitKCap, kEmitICap, kEmitMaxE, kTile = K["kEmitKCap"], K["kEmitICap"], K["kEmitMaxE"], K["kTile"]

DEC_PATHS = ("fast-lds", "fast-global", "staged-simple", "big-tables", "big-chunked")
EMIT_PATHS = ("fast", "n", "keycap", "valcap", "sizecap")  # fast, or the first predicate that fails
FAIL_N, FAIL_K, FAIL_V, FAIL_S = 1, 2, 4, 8


@dataclass
class Paths:
    """Per block: entry count, first entry, decode path (index into DEC_PATHS), the predicates'
    left-hand sides, and the emit predicates that fail (FAIL_* bits)."""
    n: np.ndarray
    first: np.ndarray
    dec: np.ndarray
    lhs_img: np.ndarray   # lead + len + 15            <= kDecImg
    lhs_out: np.ndarray   # key run + value run chunks <= kDecOut (meaningful on the fast paths)
    kb: np.ndarray        # K0 & 15, V0 & 15 of the decode output
    vb: np.ndarray
    lhs_n: np.ndarray     # n                          <= kEmitMaxE
    lhs_k: np.ndarray     # klead + KB + 8             <= kEmitKCap
    lhs_v: np.ndarray     # vlead + VB + 24            <= kEmitICap
    lhs_s: np.ndarray     # (O & 15) + size + 8        <= kEmitICap
    klead: np.ndarray
    vlead: np.ndarray
    olead: np.ndarray
    fail: np.ndarray

    @property
    def is_big(self):
        return self.fail != 0

    @property
    def emit(self):
        """Index into EMIT_PATHS: 0 fast, else the first failing predicate in the kernel's order."""
        f = self.fail
        return np.where(f == 0, 0, np.where(f & FAIL_N, 1, np.where(f & FAIL_K, 2, np.where(f & FAIL_V, 3, 4))))

    def dec_counts(self):
        return {p: int((self.dec == i).sum()) for i, p in enumerate(DEC_PATHS)}

    def emit_counts(self):
        e = self.emit
        return {p: int((e == i).sum()) for i, p in enumerate(EMIT_PATHS)}


def block_entry_counts(blocks, blk_off):
    """The u16 big-endian entry count that ends every block."""
    end = np.asarray(blk_off[1:], np.int64)
    return (blocks[end - 2].astype(np.int64) << 8) | blocks[end - 1].astype(np.int64)


def classify(blocks, blk_off, key_off, val_off, blk_addr=0, key_addr=0, val_addr=0, out_addr=0):
    """The path of every block of an oracle-encoded stream.  *_addr: the base addresses (only their
    low 4 bits matter) of the block stream read by the decode, of the key and value arenas read by
    the encode, and of the encode's output.  The decode's own output arenas and the encode's output
    are 16-byte aligned by the API (out_addr must be)."""
    assert out_addr % 16 == 0
    off = np.asarray(blk_off, np.int64)
    ko, vo = np.asarray(key_off, np.int64), np.asarray(val_off, np.int64)
    n = block_entry_counts(blocks, off)
    first = np.concatenate([[0], np.cumsum(n)])
    assert first[-1] == len(ko) - 1, "entry counts do not add up (a wrapped u16 count?)"
    s, e = first[:-1], first[1:]
    ln = off[1:] - off[:-1]
    KB, VB = ko[e] - ko[s], vo[e] - vo[s]
    # decode (decode_block, dec_fast_outputs)
    lead = (blk_addr + off[:-1]) & 15
    lhs_img = lead + ln + 15
    fits = lhs_img <= kDecImg
    kb, vb = ko[s] & 15, vo[s] & 15
    lhs_out = ((kb + KB + 15) & ~15) + ((vb + VB + 15) & ~15)
    small = n <= kDecMaxE
    dec = np.where(fits & small, np.where(lhs_out <= kDecOut, 0, 1), np.where(fits, 2, np.where(small, 3, 4)))
    # emit (is_fast)
    klead, vlead, olead = (key_addr + ko[s]) & 15, (val_addr + vo[s]) & 15, off[:-1] & 15
    lhs_k, lhs_v, lhs_s = klead + KB + 8, vlead + VB + 24, olead + ln + 8
    fail = (FAIL_N * (n > kEmitMaxE) + FAIL_K * (lhs_k > kEmitKCap) + FAIL_V * (lhs_v > kEmitICap) +
            FAIL_S * (lhs_s > kEmitICap))
    return Paths(n, s, dec, lhs_img, lhs_out, kb, vb, n, lhs_k, lhs_v, lhs_s, klead, vlead, olead, fail)


def wave_sequences(is_big, nw):
    """The fast / big string ('F' / 'B') every wave sees under the strided assignment
    w, w + nw, w + 2 nw, ... (emit_kernel, emit_big_kernel; fuse_emit per walker)."""
    fb = np.where(np.asarray(is_big, bool), ord("B"), ord("F")).astype(np.uint8)
    return [fb[w::nw].tobytes().decode() for w in range(min(int(nw), len(fb)))]


# ------------------------------------------------------------------------------- KV assembly
def _kv(klen, vlen, head, hcols, rng):
    """Random key and value bytes of the given lengths; head[:, c] overwrites key byte c of every
    entry whose key has more than c bytes, for c < hcols (the ordering prefix)."""
    klen, vlen = np.asarray(klen, np.uint64), np.asarray(vlen, np.uint64)
    assert (klen > 0).all()
    ko, vo = synth._offsets(klen), synth._offsets(vlen)
    keys = synth._random_bytes(rng, int(ko[-1]))
    vals = synth._random_bytes(rng, int(vo[-1]))
    k0 = ko[:-1].astype(np.int64)
    for c in range(hcols):
        m = klen > c
        keys[k0[m] + c] = head[m, c]
    return O.KV(keys, ko, vals, vo, synth._ts(rng, len(klen)))


def _be(x, nbytes):
    """x as nbytes big-endian byte columns (n, nbytes)."""
    x = np.asarray(x, np.uint64)
    if nbytes == 0:
        return np.zeros((len(x), 0), np.uint8)
    return np.stack([(x >> np.uint64(8 * (nbytes - 1 - c))).astype(np.uint8) for c in range(nbytes)], 1)


def kv_equal(a: O.KV, b: O.KV):
    return (a.n == b.n and np.array_equal(a.key_off, b.key_off) and np.array_equal(a.val_off, b.val_off) and
            np.array_equal(a.ts, b.ts) and np.array_equal(a.keys[:a.key_off[-1]], b.keys[:b.key_off[-1]]) and
            np.array_equal(a.vals[:a.val_off[-1]], b.vals[:b.val_off[-1]]))


# ------------------------------------------------------------------------------- stream A
A_BLOCKS_PER_WAVE = 71
A_BLOCK_SIZE = 16  # every entry its own block: block index == entry index


def emit_nws(cus, pmax):
    """The wave counts emit_kernel can have: 4 waves x CUs x workgroups per CU."""
    return [4 * cus * p for p in range(1, pmax + 1)]


def stream_a(cus, seed=101):
    """71 * NW one-entry blocks (NW = 32 * CUs bounds the waves of emit_kernel and emit_big_kernel):
    0.2 % big entries everywhere, 30 % inside one region of 6 * NW blocks, entry 0 and the last
    entry big with a fast block one stride after / before them for every wave count."""
    rng = np.random.default_rng(seed)
    NW = 32 * cus
    n = A_BLOCKS_PER_WAVE * NW
    big = rng.random(n) < 0.002
    r0 = 20 * NW
    big[r0:r0 + 6 * NW] = rng.random(6 * NW) < 0.30
    nws = np.asarray(emit_nws(cus, 8))
    big[nws] = False
    big[n - 1 - nws] = False
    big[0] = big[n - 1] = True
    bigval = big & (rng.random(n) < 0.1)
    bigval[0], bigval[n - 1] = False, True
    bigkey = big & ~bigval
    klen = np.where(bigkey, 1100, 3)
    vlen = np.where(bigval, 4300, rng.integers(0, 41, n))
    kv = _kv(klen, vlen, _be(np.arange(n), 3), 3, rng)
    cuts = np.cumsum(rng.integers(2000, 6001, n // 2000 + 1))
    seg = np.concatenate([[0], cuts[cuts < n], [n]]).astype(np.uint32)
    return kv, seg, A_BLOCK_SIZE


def check_stream_a(p: Paths, cus):
    """The conditions of stream A for a device of `cus` CUs."""
    NW = 32 * cus
    nblk = len(p.n)
    assert nblk == A_BLOCKS_PER_WAVE * NW and (p.n == 1).all(), "every entry its own block"
    big = p.is_big
    for nw in emit_nws(cus, 8):
        seqs = wave_sequences(big, nw)
        for pat in ("FBF", "FBBF", "FBBBF"):
            assert any(pat in s for s in seqs), f"nw={nw}: no wave sees {pat}"
        assert seqs[0].startswith("BF"), f"nw={nw}: wave of block 0 starts {seqs[0][:4]}"
        last = seqs[(nblk - 1) % nw]
        assert last.endswith("FB"), f"nw={nw}: wave of the last block ends {last[-4:]}"
    assert big[64 * NW:].any(), "no big block for emit_big_kernel's second ballot round"
    e = p.emit_counts()
    assert e["keycap"] > 0 and e["valcap"] > 0 and e["fast"] > 0


# ------------------------------------------------------------------------------- stream B
B_BLOCK_SIZE = 3072  # the smallest at which a block can exceed 128 entries (129 x 21 + 2 = 2711)


def stream_b_min_blocks(cus):
    return 6 * 16 * cus


def stream_b(cus, seed=202):
    """Natural packing at block_size 3072 over runs of five regimes: U-like (16-B key, 80-120-B
    value), tiny (3-B key, empty value: > 128 entries per block), long keys (40-90-B keys, 0-5-B
    values: over the key cap), oversize values (4300-6000 B) and oversize keys (1100-1400 B)."""
    rng = np.random.default_rng(seed)
    want = stream_b_min_blocks(cus)
    per_block = np.array([23, 180, 36, 1, 2])
    nrun = int(want * 1.25 / 4.5) + 8
    reg = rng.choice(5, nrun, p=[0.62, 0.10, 0.13, 0.09, 0.06])
    nb = rng.integers(1, 9, nrun)
    cnt = np.maximum(1, (per_block[reg] * nb * rng.uniform(0.8, 1.2, nrun)).astype(np.int64))
    r = np.repeat(reg, cnt)
    n = len(r)
    assert n < 1 << 24
    klen = np.choose(r, [np.full(n, 16), np.full(n, 3), rng.integers(40, 91, n), np.full(n, 16),
                         rng.integers(1100, 1401, n)])
    vlen = np.choose(r, [rng.integers(80, 121, n), np.zeros(n, np.int64), rng.integers(0, 6, n),
                         rng.integers(4300, 6001, n), rng.integers(0, 41, n)])
    kv = _kv(klen, vlen, _be(np.arange(n), 3), 3, rng)
    seg = synth.segments_by_bytes(kv.key_off, kv.val_off, 256 << 10)
    return kv, seg, B_BLOCK_SIZE


def check_stream_b(p: Paths, cus):
    nblk = len(p.n)
    assert nblk >= stream_b_min_blocks(cus), nblk
    f = p.fail
    only_n, only_k, val_or_size = (f == FAIL_N).sum(), (f == FAIL_K).sum(), ((f & (FAIL_V | FAIL_S)) != 0).sum()
    assert only_n >= 0.01 * nblk and only_k >= 0.01 * nblk and val_or_size >= 0.01 * nblk, (only_n, only_k, val_or_size)
    assert (f == 0).sum() >= 0.5 * nblk, (f == 0).sum()
    for nw in emit_nws(cus, 4):
        seqs = wave_sequences(p.is_big, nw)
        for pat in ("FBF", "FBBF"):
            assert any(pat in s for s in seqs), f"nw={nw}: no wave sees {pat}"


# ------------------------------------------------------------------------------- probe lists
class _Probes:
    """One segment per probe.  Keys are [probe index BE u16][entry index][random ...]: sorted over
    the list, and inside a probe every key shares exactly `shared` bytes with the probe's first."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.kl, self.vl, self.ent, self.pidx = [], [], [], []

    def add(self, klen, vlen):
        klen, vlen = np.asarray(klen, np.int64), np.asarray(vlen, np.int64)
        assert len(klen) == len(vlen) and (klen > 0).all() and (vlen >= 0).all() and len(self.kl) < 65536
        self.ent.append(np.arange(len(klen)))
        self.pidx.append(np.full(len(klen), len(self.kl)))
        self.kl.append(klen)
        self.vl.append(vlen)

    def build(self, block_size, ent_bytes=1):
        klen, vlen = np.concatenate(self.kl), np.concatenate(self.vl)
        head = np.concatenate([_be(np.concatenate(self.pidx), 2), _be(np.concatenate(self.ent), ent_bytes)], 1)
        kv = _kv(klen, vlen, head, 2 + ent_bytes, self.rng)
        seg = np.concatenate([[0], np.cumsum([len(k) for k in self.kl])]).astype(np.uint32)
        return kv, seg, block_size


def _spread(total, n):
    """n non-negative lengths that add up to total, as even as possible."""
    assert total >= 0
    return total // n + (np.arange(n) < total % n)


EMIT_COUNT_NS = (1, 2, 63, 64, 65, 127, 128, 129, 130)


def probes_emit_count(seed=301):
    """Tiny entries (3-B key, empty value): only the entry count moves."""
    P = _Probes(seed)
    for n in EMIT_COUNT_NS:
        P.add(np.full(n, 3), np.zeros(n))
    return P.build(4096)


def probes_emit_keycap(seed=302):
    """20-entry blocks whose key bytes KB take every value in [kEmitKCap - 40, kEmitKCap + 8]."""
    P = _Probes(seed)
    for KB in range(kEmitKCap - 40, kEmitKCap + 9):
        P.add(_spread(KB, 20), np.zeros(20))
    return P.build(4096)


def _cap_sweep():
    """Value totals v of a cap sweep (each block v + 19 bytes): +-17 around the cap after the slack
    and any lead 0..15, in three orders (up, down, shuffled), so that the value arena's alignments
    meet every length; then one block for every target of the size cap's left-hand side, its length
    chosen for the output offset it lands on (O & 15 follows the sizes before it)."""
    base = np.arange(kEmitICap - 17 - 27 - 15 - 20, kEmitICap + 17 - 24 + 4)
    v = np.concatenate([base, base[::-1], np.random.default_rng(7).permutation(base)]).tolist()
    out = int(sum(v)) + 19 * len(v)
    for t in range(kEmitICap - 17, kEmitICap + 18):
        v.append(t - 8 - 19 - (out & 15))
        out += v[-1] + 19
    return np.asarray(v)


def probes_emit_valcap(seed=303):
    """Single-entry blocks, 1-byte key: VB = vlen, size = vlen + 19, both caps swept."""
    P = _Probes(seed)
    for v in _cap_sweep():
        P.add([1], [v])
    kv, seg, bs = P.build(4096, ent_bytes=0)
    kv.keys[:] = (np.arange(kv.n) * 256 // kv.n).astype(np.uint8)  # (1-byte keys: non-decreasing)
    return kv, seg, bs


def probes_emit_sizecap(seed=304):
    """20-entry blocks with 50-B keys: KB = 1000 and VB ~ 2900 stay clear of their caps, the
    encoded size sweeps its own.  block_size 8192 (no fused run)."""
    P = _Probes(seed)
    for v in _cap_sweep():
        # size = 16 per entry + key suffixes (50, then 48 each) + values + 2; v + 19 as the single entries'
        P.add(np.full(20, 50), _spread(int(v) + 19 - (20 * 16 + 50 + 19 * 48 + 2), 20))
    return P.build(8192)


DEC_STAGED_LENS = range(kDecImg - 48, kDecImg + 17)


def probes_dec_staged(seed=305):
    """Blocks of 1, 2 and 128 entries at every length in [kDecImg - 48, kDecImg + 16]
    (block_size 8192: a second entry must fit the builder's estimate)."""
    P = _Probes(seed)
    for n in (1, 2, 128):
        for ln in DEC_STAGED_LENS:
            # len = 16 n + suffixes (3, then 1 each) + values + 2
            P.add(np.full(n, 3), _spread(ln - (17 * n + 4), n))
    return P.build(8192)


DEC_COUNT_NS = (63, 64, 65, 127, 128, 129, 130, 191, 192, 193, 256, 257)
# a staged block has lead + len + 15 <= kDecImg and an entry takes >= 16 bytes
DEC_COUNT_STAGED_MAX = (kDecImg - 15 - 2 - 1) // 16


def probes_dec_count(seed=306):
    """Entry counts around kDecMaxE and its multiples, staged and unstaged.  Staged: distinct 4-B
    keys, but from 200 entries on one 1-byte key in many versions (16 B per entry), that block
    first in the stream (lead = the stream's own); 257 entries cannot be staged at all
    (257 x 16 + 3 > kDecImg - 15).  Unstaged: the first value is 4200 B."""
    P = _Probes(seed)
    staged = [n for n in DEC_COUNT_NS if n <= DEC_COUNT_STAGED_MAX]
    for n in sorted(staged, key=lambda n: n < 200):
        P.add(np.full(n, 4 if n < 200 else 1), np.zeros(n))
    for n in DEC_COUNT_NS:
        P.add(np.full(n, 4), np.concatenate([[kDecImg + 72], np.zeros(n - 1)]))
    kv, seg, bs = P.build(16384, ent_bytes=2)
    for g in range(len(staged)):  # the many-version blocks: every key the same single byte
        if kv.key_off[seg[g] + 1] - kv.key_off[seg[g]] == 1:
            kv.keys[kv.key_off[seg[g]]:kv.key_off[seg[g + 1]]] = g
    return kv, seg, bs, len(staged)


OUT_LEADS = (0, 1, 8, 15)


def probes_dec_outimage(seed=307):
    """Staged 30-entry blocks with 102-B keys sharing 100 bytes (K = 3060, block ~1.6 KB), V swept
    so that K + V covers [kDecOut - 48, kDecOut + 16]; before each, a one-entry filler block that
    sets the output offsets' low bits (K0 & 15, V0 & 15) to every pair from OUT_LEADS."""
    P = _Probes(seed)
    Kc = Vc = 0
    shared = []
    for kb in OUT_LEADS:
        for vb in OUT_LEADS:
            for V in range(kDecOut - 48 - 3060, kDecOut + 17 - 3060):
                fk, fv = (kb - Kc - 2) % 16 + 2, (vb - Vc) % 16
                P.add([fk], [fv])
                shared.append(False)
                P.add(np.full(30, 102), _spread(V, 30))
                shared.append(True)
                Kc, Vc = Kc + fk + 3060, Vc + fv + V
    kv, seg, bs = P.build(4096)
    # bytes 3..99 of a probe's keys: those of its first key (the entry index moves to byte 100)
    k = kv.keys
    for g in np.flatnonzero(shared):
        rows = k[kv.key_off[seg[g]]:kv.key_off[seg[g + 1]]].reshape(30, 102)
        rows[:, 100] = rows[:, 2]
        rows[:, 2:100] = rows[0, 2:100]
    return kv, seg, bs


def one_block_per_segment(blk_off, seg):
    return len(blk_off) - 1 == len(seg) - 1


def both_sides(lhs, cap, near=None):
    """lhs takes the value cap and the value cap + 1 (near=None), or some value in
    [cap - near, cap] and some in (cap, cap + near]."""
    lhs = np.asarray(lhs)
    if near is None:
        return bool((lhs == cap).any() and (lhs == cap + 1).any())
    return bool(((lhs <= cap) & (lhs >= cap - near)).any() and ((lhs > cap) & (lhs <= cap + near)).any())


def coverage_line(name, p: Paths):
    """One line for a log: the block counts per path and the predicates' ranges by side."""
    def side(lhs, cap):
        lo, hi = lhs[lhs <= cap], lhs[lhs > cap]
        return f"<=:{lo.min() if lo.size else '-'}..{lo.max() if lo.size else '-'} >:{hi.min() if hi.size else '-'}..{hi.max() if hi.size else '-'}"
    fast = p.dec <= 1
    return (f"{name}: {len(p.n)} blocks; decode {p.dec_counts()}; emit {p.emit_counts()}; "
            f"img[{side(p.lhs_img, kDecImg)}] decn[{side(p.n, kDecMaxE)}] "
            f"out[{side(p.lhs_out[fast], kDecOut) if fast.any() else '-'}] n[{side(p.lhs_n, kEmitMaxE)}] "
            f"k[{side(p.lhs_k, kEmitKCap)}] v[{side(p.lhs_v, kEmitICap)}] s[{side(p.lhs_s, kEmitICap)}]")
