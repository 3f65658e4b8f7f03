"""Inputs that put byte ranges on chosen paths of the CRC-32 kernels -- TEST INFRASTRUCTURE.

The method of path_cases.py and sst_cases.py, for crc_stream_kernel (the plain pass of
lsmblk_crc32_batch, the lagged verifying decode and the framed encode) and crc_kernel<COUNT> (the
two-pass verifying decode's fused count, the section CRCs); shared by test_crc_cases.py (CPU) and
test_gpu_crc_paths.py (GPU):

  constants    kCrcChunk, kCrcSeg, kCrcPad, kCsWaves read out of the kernel sources; the probes
               are derived from them.  (crc_stream_kernel writes its own 4-KiB chunk as the
               literals 4095 and 12: STREAM_CHUNK restates them.)
  models       numpy / Python restatements of what picks a path: per block of the streaming kernel
               T, nch, P, the byte path and the shifted last piece, per wave nb, maxnch and
               wave_ok, the launch rule's groups per wave; per chunk of crc_kernel lead, sz, tz,
               the load piece, nseg and r, and where the count reads.  They only ASSERT COVERAGE;
               expected CRCs come from zlib / oracle.crc32, expected blocks and streams from
               oracle/ alone.
  generators   a-f below.  All data is random with the first and last byte of every block
               non-zero, and every byte outside the blocks (before the first, after the last, the
               gaps) is random and non-zero: one byte read too many, or one masked too few,
               changes the CRC.

A check_* function takes the constants it checks against, so a case built for other constants
fails it.
"""
import os
import zlib
from dataclasses import dataclass, field

import numpy as np

import path_cases as pc
from oracle import oracle as O
from oracle import pyref

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsm_amd", "csrc")
SOURCES = {"kCrcChunk": "lsmblk_dev.hpp", "kCrcSeg": "lsmblk_dev.hpp", "kCrcPad": "lsmblk_dev.hpp",
           "kCsWaves": "lsmblk_gpu.hip"}


@dataclass(frozen=True)
class Consts:
    kCrcChunk: int
    kCrcSeg: int
    kCrcPad: int
    kCsWaves: int

    @property
    def full_segs(self):
        """Whole lane windows in a chunk (60 today)."""
        return self.kCrcChunk // self.kCrcSeg


def kernel_constants(path=None):
    """The CRC kernels' constants, read the way sst_cases.kernel_constants reads its own.  path:
    {constant: source file} for those to be read from a retuned scratch copy."""
    path = path or {}
    out = {}
    for name, src in SOURCES.items():
        out.update(pc.read_constants(path.get(name, os.path.join(_CSRC, src)), (name,)))
    return Consts(**out)


C = kernel_constants()
STREAM_CHUNK = 4096          # crc_stream_kernel: `(L + T + 4095) >> 12`
MAX_RANGE = 0x7FFFFFF0       # the largest range either kernel accepts
ERR_MALFORMED = 1            # LSMBLK_ERR_MALFORMED, the stats[3] flag
GUARD = 64                   # random non-zero bytes on either side of a placed stream (a multiple of 16)
NOMINAL_CUS = 256
LOAD_PIECE = 1024            # crc_kernel's issue(): five loads of 64 lanes x 16 B per chunk


# ------------------------------------------------------------------------------- bytes and places
def _nonzero(rng, n):
    return rng.integers(1, 256, n, dtype=np.uint8)


@dataclass
class Ranges:
    """Ranges [off[b], off[b + 1]) of `body`, of which the last `tail` bytes are not block."""
    body: np.ndarray          # u8
    off: np.ndarray           # i64[nblk + 1]
    tail: int

    @property
    def nblk(self):
        return len(self.off) - 1

    def lens(self):
        return np.diff(self.off) - self.tail

    def block(self, b):
        return self.body[int(self.off[b]):int(self.off[b + 1]) - self.tail].tobytes()

    def prefix(self, n):
        """The first n ranges; the bytes of the later ones stay behind them."""
        return Ranges(self.body, self.off[:n + 1], self.tail)


def random_ranges(lens, tail, rng, edges=None):
    """Blocks of the given lengths back to back, each followed by `tail` random non-zero bytes;
    block bytes random, the first and last of each non-zero, and so the bytes on either side of
    every chunk edge (edges(L) -> block offsets)."""
    lens = np.asarray(lens, np.int64)
    off = np.concatenate([[0], np.cumsum(lens + tail)]).astype(np.int64)
    body = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    nz = lens > 0
    body[off[:-1][nz]] = _nonzero(rng, int(nz.sum()))
    body[(off[:-1] + lens - 1)[nz]] = _nonzero(rng, int(nz.sum()))
    for k in range(tail):
        body[off[:-1] + lens + k] = _nonzero(rng, len(lens))
    for b in np.flatnonzero(lens > (STREAM_CHUNK - 16 if edges else 1 << 62)):
        at = np.array([int(off[b]) + x - d for x in edges(int(lens[b])) for d in (1, 0)], np.int64)
        body[at] = _nonzero(rng, len(at))
    return Ranges(body, off, tail)


def placed(body, shift, seed=0):
    """-> (image, start): `body` at image[start:], start = GUARD + shift, between GUARD or more
    random non-zero bytes on either side.  The image goes to a 16-byte aligned device buffer, so
    the stream's address is `shift` mod 16."""
    assert 0 <= shift < 16 and GUARD % 16 == 0
    rng = np.random.default_rng(1000 + 16 * seed + shift)
    start = GUARD + shift
    img = _nonzero(rng, start + len(body) + GUARD)
    img[start:start + len(body)] = body
    return img, start


def expected_crcs(r: Ranges, crc=zlib.crc32):
    """-> (u32[nblk] CRCs, refused bool[nblk]) by the header's contract: a range shorter than tail,
    decreasing or over MAX_RANGE is refused and its CRC is 0; an empty block's CRC is 0."""
    s, e = r.off[:-1], r.off[1:]
    refused = (e < s + r.tail) | (e - s > MAX_RANGE)
    out = np.zeros(r.nblk, np.uint32)
    for b in np.flatnonzero(~refused):
        out[b] = crc(r.block(b))
    return out, refused


def framed(blocks, blk_off):
    """The SST data section of packed blocks: block || zlib.crc32 big-endian, per block."""
    off = np.asarray(blk_off, np.int64)
    nb = len(off) - 1
    foff = off + 4 * np.arange(nb + 1)
    body = np.zeros(int(foff[-1]), np.uint8)
    for b in range(nb):
        blk = blocks[int(off[b]):int(off[b + 1])]
        body[int(foff[b]):int(foff[b]) + len(blk)] = blk
        body[int(foff[b + 1]) - 4:int(foff[b + 1])] = np.frombuffer(zlib.crc32(blk.tobytes()).to_bytes(4, "big"), np.uint8)
    return Ranges(body, foff, 4)


# ------------------------------------------------------------------------------- crc_stream_kernel
@dataclass
class StreamBlocks:
    """Per block, as crc_stream_kernel computes them from blk_off and tail."""
    valid: np.ndarray
    L: np.ndarray
    T: np.ndarray        # zero bytes after the message up to a multiple of 16
    nch: np.ndarray
    P: np.ndarray        # zero bytes before the message: fills the first chunk
    byte_path: np.ndarray   # L < 16: the last piece by byte loads
    shifted: np.ndarray     # L >= 16 && T != 0: the block's last 16 bytes, down by T


def stream_blocks(off, tail):
    off = np.asarray(off, np.int64)
    s, e = off[:-1], off[1:]
    valid = (e >= s + tail) & (e - s <= MAX_RANGE)
    L = np.where(valid, e - s - tail, 0)
    T = -L & 15
    nch = (L + T + STREAM_CHUNK - 1) // STREAM_CHUNK
    P = nch * STREAM_CHUNK - L - T
    return StreamBlocks(valid, L, T, nch, P, valid & (L < 16) & (T != 0), (L >= 16) & (T != 0))


@dataclass
class StreamWaves:
    """Per wave (group of four consecutive blocks)."""
    nb: np.ndarray
    maxnch: np.ndarray
    idle: np.ndarray       # rows with a block whose nch < maxnch (they run dead chunks)
    wave_ok: np.ndarray    # one descriptor over [S0, Se); false: one per block


def stream_waves(off, tail):
    """wave_ok exactly as the kernel computes it: Se >= S0, Se - S0 within MAX_RANGE, and no valid
    row with s < S0 or s + L > Se."""
    off = [int(x) for x in off]
    b = stream_blocks(off, tail)
    nblk = len(off) - 1
    nb, maxnch, idle, ok = [], [], [], []
    for b0 in range(0, nblk, 4):
        n = min(4, nblk - b0)
        S0, Se = off[b0], off[b0 + n]
        out = any(b.valid[b0 + g] and (off[b0 + g] < S0 or off[b0 + g] + int(b.L[b0 + g]) > Se) for g in range(n))
        m = int(b.nch[b0:b0 + n].max())
        nb.append(n)
        maxnch.append(m)
        idle.append(int((b.nch[b0:b0 + n] < m).sum()))
        ok.append(Se >= S0 and Se - S0 <= MAX_RANGE and not out)
    return StreamWaves(np.array(nb), np.array(maxnch), np.array(idle), np.array(ok, bool))


def stream_launch(nblk, cus, c=C):
    """launch_crc's grid for crc_stream_kernel -> (workgroups, waves, groups, groups per wave)."""
    per = 4 * c.kCsWaves
    want = (nblk + per - 1) // per
    grid = min(max(want, 1), cus)
    nw, ngrp = grid * c.kCsWaves, (nblk + 3) // 4
    return grid, nw, ngrp, np.array([len(range(w, ngrp, nw)) for w in range(nw)])


def stream_edges(L):
    """Data offsets at which a chunk of the padded message 0^P || M || 0^T ends inside M."""
    T = -L & 15
    nch = (L + T + STREAM_CHUNK - 1) // STREAM_CHUNK
    P = nch * STREAM_CHUNK - L - T
    return [STREAM_CHUNK * c - P for c in range(1, nch)]


# a. streaming lengths
def stream_lengths():
    """[0, 272], 4096 k +- 40 for k = 1, 2, 3, [65520, 65553]: 550 lengths."""
    return (list(range(0, 273)) + [STREAM_CHUNK * k + d for k in (1, 2, 3) for d in range(-40, 41)] +
            list(range(65520, 65554)))


EXTRA_EMPTY = 3   # empty blocks beside the one of stream_lengths(): one for each row position


def stream_case(tail=0, seed=501, lengths=None):
    """The lengths of stream_lengths() and EXTRA_EMPTY more empty blocks, shuffled (rows of one
    wave differ in nch), then steered: wave 0 holds nch = 0, 1, 2 and >= 3 with its empty block in
    row 0, and waves 1, 2, 3 have an empty block in rows 1, 2, 3."""
    rng = np.random.default_rng(seed)
    ls = list(stream_lengths() if lengths is None else lengths)
    ls = [ls[i] for i in rng.permutation(len(ls))]

    def take(lo, hi):
        i = next(i for i, x in enumerate(ls) if lo <= x <= hi)
        return ls.pop(i)
    head = [take(0, 0), take(1, STREAM_CHUNK), take(STREAM_CHUNK + 1, 2 * STREAM_CHUNK), take(2 * STREAM_CHUNK + 1, 1 << 30)]
    for g in (1, 2, 3):
        row = [ls.pop(0) for _ in range(3)]
        row.insert(g, 0)
        head += row
    return random_ranges(head + ls, tail, rng, stream_edges)


def stream_counts(nblk):
    """The batch sizes (a) runs at: whole, cut to the other three residues mod 4, one block."""
    return [nblk, nblk - 1, nblk - 2, nblk - 3, 1]


def check_stream_case(r: Ranges):
    b = stream_blocks(r.off, r.tail)
    w = stream_waves(r.off, r.tail)
    L, T = b.L, b.T
    assert b.valid.all() and w.wave_ok.all()
    assert set(T[L >= 16].tolist()) == set(range(16)), "every T with L >= 16"
    assert set(T[(L < 16) & (L > 0)].tolist()) == set(range(1, 16)), "every non-zero T on the byte path"
    assert 16 in L and 0 in L
    assert b.byte_path.sum() == 15 and b.shifted.any() and ((L >= 16) & (T == 0)).any()
    assert 0 in b.P[b.nch > 0] and STREAM_CHUNK - 16 in b.P, "P = 0 and P = 4080"
    for k in (1, 2, 3):   # both sides of the chunk edges nch k -> k + 1
        lo, hi = b.nch[L == k * STREAM_CHUNK], b.nch[L == k * STREAM_CHUNK + 1]
        assert lo.size and hi.size and (lo == k).all() and (hi == k + 1).all(), f"chunk edge {k}"
        # ... and of the T that carries a length over it
        assert (b.nch[(L > k * STREAM_CHUNK - 16) & (L <= k * STREAM_CHUNK)] == k).all()
    rows = {g for g in range(4) if (L[g::4] == 0).any()}
    assert rows == {0, 1, 2, 3}, f"an empty block in every row position: {rows}"
    nch4 = [sorted(np.minimum(b.nch[i:i + 4], 3).tolist()) for i in range(0, r.nblk - 3, 4)]
    assert [0, 1, 2, 3] in nch4, "a wave with nch 0, 1, 2 and >= 3"
    mixed = int((w.idle > 0).sum())
    assert mixed >= len(w.nb) // 2, "rows of one wave differ in nch"
    assert {n % 4 for n in stream_counts(r.nblk)} == {0, 1, 2, 3} and 1 in stream_counts(r.nblk)
    return (f"{r.nblk} blocks, tail {r.tail}: T {len(set(T[L >= 16].tolist()))} values at L >= 16, "
            f"{int(b.byte_path.sum())} on the byte path; nch up to {int(b.nch.max())}; "
            f"{mixed} of {len(w.nb)} waves with maxnch > nch rows; wave_ok == false waves {int((~w.wave_ok).sum())}")


# b. streaming persistent loop
def persistent_stream_nblk(cus, c=C):
    return 2 * 4 * c.kCsWaves * cus + 4 * c.kCsWaves * 3 + 3


def persistent_stream_case(cus, c=C, seed=502):
    rng = np.random.default_rng(seed)
    return random_ranges(rng.integers(0, 41, persistent_stream_nblk(cus, c)), 0, rng)


def check_persistent_stream(nblk, cus, c=C):
    grid, nw, ngrp, per = stream_launch(nblk, cus, c)
    assert grid == cus, "one workgroup per CU"
    assert set(per.tolist()) == {2, 3}, f"every wave takes two groups, some three: {sorted(set(per.tolist()))}"
    assert int((per == 3).sum()) == 3 * c.kCsWaves + 1
    assert nblk % 4 == 3, "the last group is partial"
    # a wave issues offs(G + nw) in every pass of the loop: in its last pass G + nw >= ngrp (the
    # guarded zero), and the partial last group is fetched by that prefetch, not by the first offs(G)
    last = np.array([w + nw * (per[w] - 1) for w in range(nw)])
    assert (last + nw >= ngrp).all() and (last < ngrp).all()
    assert ngrp - 1 >= nw, "the partial group is a prefetched one"
    return (f"{nblk} blocks on {cus} CUs: {grid} workgroups, {nw} waves, {ngrp} groups; waves with two or more "
            f"groups {int((per >= 2).sum())}, with three {int((per == 3).sum())}; last group of {nblk % 4}")


# c. streaming fallback and errors
@dataclass
class ErrCase:
    name: str
    off: list
    tail: int
    span: int                 # bytes of the buffer the valid ranges lie in
    wave_ok: list = None      # what the model must say, per wave (None: not stated)


def _drop(g):
    """Eight ranges of 40 bytes from 300 on, the second wave's row g stepping back by 250."""
    lens = [40] * 8
    lens[4 + g] = -250
    return np.concatenate([[300], 300 + np.cumsum(lens)]).tolist()


def _short(short, at):
    """Ranges under tail 4 that hold blocks of 30, 9, 25, 17, 8, 1 and 33 bytes, and at index `at` one of
    `short` bytes in all."""
    lens = [34, 13, 29, 21, 12, 5, 37]
    lens.insert(at, short)
    return np.concatenate([[0], np.cumsum(lens)]).tolist()


def error_cases():
    out = []
    for tail in (0, 4):
        out.append(ErrCase(f"Se<S0 tail{tail}", [100, 200, 0, 50, 60], tail, 200, [False]))
        out.append(ErrCase(f"valid below S0 tail{tail}", [50, 100, 0, 200, 300], tail, 300, [False]))
        for g in range(4):
            out.append(ErrCase(f"step back in row {g} tail{tail}", _drop(g), tail, 700, [True, False]))
        # only the offsets are large: nothing is allocated for the refused last range
        out.append(ErrCase(f"over 2 GiB last tail{tail}", [0, 30, 70, 70 + MAX_RANGE + 1], tail, 70, [False]))
        out.append(ErrCase(f"over 2 GiB last of a second wave tail{tail}",
                           [0, 30, 70, 75, 111, 140, 140 + MAX_RANGE + 1], tail, 140, [True, False]))
    for short in range(4):
        out.append(ErrCase(f"{short} bytes under tail 4", _short(short, 4 + short), 4, 200, [True, True]))
    out.append(ErrCase("4 bytes under tail 4", _short(4, 5), 4, 200, [True, True]))
    return out


def error_ranges(ec: ErrCase, seed=503):
    """Random non-zero bytes under the valid ranges (they may overlap: any bytes will do)."""
    rng = np.random.default_rng(seed)
    return Ranges(_nonzero(rng, ec.span), np.asarray(ec.off, np.int64), ec.tail)


def check_error_cases(cases):
    flagged = clean = 0
    rows = set()
    for ec in cases:
        r = error_ranges(ec)
        b, w = stream_blocks(r.off, r.tail), stream_waves(r.off, r.tail)
        if ec.wave_ok is not None:
            assert w.wave_ok.tolist() == ec.wave_ok, (ec.name, w.wave_ok)
        s = r.off[:-1][b.valid]
        assert (s >= 0).all() and (s + b.L[b.valid] <= ec.span).all(), f"{ec.name}: a valid range leaves the buffer"
        assert (b.L[~b.valid] == 0).all() and (b.nch[~b.valid] == 0).all()   # refused: nothing is loaded
        rows |= {int(i) % 4 for i in np.flatnonzero(~b.valid)}
        flagged += bool((~b.valid).any())
        clean += bool(b.valid.all())
    assert rows == {0, 1, 2, 3} and flagged and clean
    names = [ec.name for ec in cases]
    assert len(set(names)) == len(names)
    four = next(ec for ec in cases if ec.name == "4 bytes under tail 4")
    b = stream_blocks(four.off, 4)
    assert b.valid.all() and 0 in b.L
    return f"{len(cases)} batches, {flagged} with a refused range, refused rows {sorted(rows)}"


# ------------------------------------------------------------------------------- crc_kernel
@dataclass
class Chunks:
    """Per chunk of crc_kernel, in the order it folds them."""
    blk: np.ndarray
    first: np.ndarray     # the block's first chunk (the short one)
    lead: np.ndarray      # address & 15
    sz: np.ndarray
    tz: np.ndarray        # zero bytes after the chunk up to a 4-aligned LDS address
    piece: np.ndarray     # (lead + sz) >> 10: the 1-KiB load piece the tail mask falls in
    nseg: np.ndarray
    r: np.ndarray         # the first lane window's bytes
    glob: np.ndarray      # the block's count reads global memory (nch > 1)


def kernel_chunks(addr, lens, c=C):
    """addr: every block's address (any base that is right mod 16); lens: block lengths > 0."""
    addr, lens = np.asarray(addr, np.int64), np.asarray(lens, np.int64)
    assert (lens > 0).all()
    K = c.kCrcChunk
    nch = (lens + K - 1) // K
    h = lens - K * (nch - 1)
    blk = np.repeat(np.arange(len(lens)), nch)
    idx = np.arange(int(nch.sum())) - np.repeat(np.cumsum(nch) - nch, nch)
    first = idx == 0
    start = addr[blk] + np.where(first, 0, h[blk] + K * (idx - 1))
    sz = np.where(first, h[blk], K)
    lead = start & 15
    P = lead + sz
    tz = -P & 3
    sx = sz + tz
    nseg = (sx + c.kCrcSeg - 1) // c.kCrcSeg
    return Chunks(blk, first, lead, sz, tz, P >> 10, nseg, sx - c.kCrcSeg * (nseg - 1), (nch > 1)[blk])


def kernel_edges(L, c=C):
    """Block offsets at which a chunk of crc_kernel ends inside the block."""
    nch = (L + c.kCrcChunk - 1) // c.kCrcChunk
    h = L - c.kCrcChunk * (nch - 1)
    return [h + c.kCrcChunk * k for k in range(nch - 1)]


def kernel_launch(nblk, cus, per_cu):
    """launch_crc's persistent grid for crc_kernel -> blocks per wave."""
    grid = min((nblk + 3) // 4, cus * per_cu)
    return np.array([len(range(w, nblk, 4 * grid)) for w in range(4 * grid)])


def check_chunks(chunk_sets, c=C, what="", section=False):
    """chunk_sets: the Chunks of every placement.  Every (lead, tz) pair, load pieces 0..4 (the last
    under a tail mask), nseg 1, 2, full_segs and full_segs + 1 with r on both window edges, first chunks
    of 1, kCrcChunk - 1 and kCrcChunk bytes, the count on both sides of nch <= 1."""
    cat = lambda f: np.concatenate([getattr(s, f) for s in chunk_sets])
    lead, tz, piece, nseg, r, sz, first, glob = (cat(f) for f in ("lead", "tz", "piece", "nseg", "r", "sz", "first", "glob"))
    sx = sz + tz
    pairs = set(zip(lead.tolist(), tz.tolist()))
    assert len(pairs) == 64, f"{what}: (lead, tz) pairs {len(pairs)}"
    top = (c.kCrcChunk + 15) // LOAD_PIECE   # 4 today: a whole chunk behind a lead
    assert set(piece.tolist()) == set(range(top + 1)), f"{what}: load pieces {sorted(set(piece.tolist()))}"
    assert ((piece == top) & (tz != 0)).any(), "the tail mask in the last load piece"
    F, S = c.full_segs, c.kCrcSeg
    assert F * S <= c.kCrcChunk < (F + 1) * S and c.kCrcChunk + 3 <= 64 * S
    assert {1, 2, F, F + 1} <= set(nseg.tolist()), f"{what}: nseg {sorted(set(nseg.tolist()))[:4]}.."
    for k in (1, F):   # sx = 68 k: nseg k, r = 68; sx = 68 k + 4: nseg k + 1, r = 4
        assert ((sx == S * k) & (nseg == k) & (r == S)).any(), f"{what}: r = kCrcSeg at nseg {k}"
        assert ((sx == S * k + 4) & (nseg == k + 1) & (r == 4)).any(), f"{what}: r = 4 at nseg {k + 1}"
    assert ((nseg == 1) & (r <= 4)).any() and ((nseg == 2) & (r == S)).any()
    assert {1, c.kCrcChunk - 1, c.kCrcChunk} <= set(sz[first].tolist()), f"{what}: first chunks of 1, K - 1, K bytes"
    assert (~first).any() and (sz[~first] == c.kCrcChunk).all()
    # dead lanes read kCrcSeg bytes before the chunk, lane l0 up to kCrcSeg - r: inside the zero pad
    assert c.kCrcSeg <= c.kCrcPad and c.kCrcPad % 16 == 0
    assert glob.any() and (~glob).any(), f"{what}: the count on both sides of nch <= 1"
    return (f"{what}: {len(lead)} chunks over {len(chunk_sets)} placements; (lead, tz) pairs {len(pairs)}; load pieces "
            f"{sorted(set(piece.tolist()))}; nseg {int(nseg.min())}..{int(nseg.max())}; r {int(r.min())}..{int(r.max())}; "
            f"blocks counted from {'LDS' if not section else 'one chunk'} {int((first & ~glob).sum())}, from "
            f"{'global memory' if not section else 'more'} {int((first & glob).sum())}")


def probe_lengths(lo, windows, spread, c=C):
    """[lo, lo + 280], kCrcChunk k +- spread for k in windows, the window edges the constants put
    elsewhere (today all inside those): kCrcSeg k and + 4 for k = 1, 2, full_segs; and the lengths
    that put lead + sz on either side of the load pieces' edges (LOAD_PIECE p - 20 .. + 4)."""
    K, S, F = c.kCrcChunk, c.kCrcSeg, c.full_segs
    out = set(range(lo, lo + 281))
    for k in windows:
        out |= set(range(K * k - spread, K * k + spread + 1))
    for k in (1, 2, F):
        out |= {x for x in range(S * k - 4, S * k + 9) if x >= lo}
    for p in range(1, (K + LOAD_PIECE - 1) // LOAD_PIECE):
        out |= set(range(LOAD_PIECE * p - 20, LOAD_PIECE * p + 5))
    return sorted(out)


# d. one-entry blocks of a chosen length
BLOCK_BS = 16384
MANY_ENTRIES = (100, 40)   # a block of more than 64 entries and one of 64 or fewer, both over one chunk


@dataclass
class BlockCase:
    kv: O.KV
    seg: np.ndarray
    bs: int
    blocks: np.ndarray = None
    blk_off: np.ndarray = None
    tag: list = field(default_factory=list)     # per block: its length, or ("entries", n)

    def encode(self):
        rc, self.blocks, self.blk_off = O.encode_segments(self.kv, self.seg, self.bs)
        assert rc == 0 and len(self.blk_off) == len(self.seg), "one block per segment"
        return self

    def lens(self):
        return np.diff(self.blk_off.astype(np.int64))

    def framed(self):
        return framed(self.blocks, self.blk_off)


def _block_kv(specs, rng, order=True):
    """specs: per segment (key lengths, value lengths).  Every key, value and ts byte is random and
    non-zero, so a block's zero bytes are those its format fixes.  order: the keys of a segment of
    several entries (of two bytes or more each) start with the entry's index in it, in base 250."""
    klen = np.concatenate([np.asarray(k, np.int64) for k, _ in specs])
    vlen = np.concatenate([np.asarray(v, np.int64) for _, v in specs])
    assert (klen > 0).all()
    ko = np.concatenate([[0], np.cumsum(klen)]).astype(np.uint32)
    vo = np.concatenate([[0], np.cumsum(vlen)]).astype(np.uint32)
    keys, vals = _nonzero(rng, int(ko[-1])), _nonzero(rng, int(vo[-1]))
    seg = np.concatenate([[0], np.cumsum([len(k) for k, _ in specs])]).astype(np.uint32)
    for a, b in zip(seg[:-1].tolist(), seg[1:].tolist()):
        if order and b - a > 1:
            assert (klen[a:b] >= 2).all() and b - a <= 250 * 250
            i = np.arange(b - a)
            keys[ko[a:b].astype(np.int64)] = 1 + i // 250
            keys[ko[a:b].astype(np.int64) + 1] = 1 + i % 250
    return O.KV(keys, ko, vals, vo, _nonzero(rng, 8 * len(klen)).view(np.uint64)), seg


def _one_entry(L, rng):
    """(key length, value length) of a one-entry block of L = 18 + klen + vlen bytes."""
    k = int(rng.integers(1, min(40, L - 18) + 1))
    return [k], [L - 18 - k]


def block_case(c=C, seed=504):
    """One-entry blocks of the lengths [19, 299], kCrcChunk k +- 80 (k = 1, 2, 3) and the load piece
    edges (probe_lengths), shuffled, with
    a multi-chunk block first, in the middle and last, and after the middle one the two blocks of
    MANY_ENTRIES."""
    rng = np.random.default_rng(seed)
    ls = probe_lengths(19, (1, 2, 3), 80, c)
    ls = [ls[i] for i in rng.permutation(len(ls))]
    big = [i for i, x in enumerate(ls) if x > c.kCrcChunk][:3]
    ends = [ls[i] for i in big]
    rest = [x for i, x in enumerate(ls) if i not in big]
    mid = len(rest) // 2
    order = [ends[0]] + rest[:mid] + [ends[1], ("entries", MANY_ENTRIES[0]), ("entries", MANY_ENTRIES[1])] + rest[mid:] + [ends[2]]
    specs = []
    for x in order:
        if isinstance(x, tuple):
            n = x[1]
            specs.append((rng.integers(4, 20, n), rng.integers((2 * c.kCrcChunk) // n, (3 * c.kCrcChunk) // n, n)))
        else:
            specs.append(_one_entry(x, rng))
    kv, seg = _block_kv(specs, rng)
    return BlockCase(kv, seg, BLOCK_BS, tag=order).encode()


def victims(case: BlockCase, c=C):
    """Blocks whose bytes the verifying decode's flips go to: the first, the one at the middle
    index and the last, all over one chunk."""
    n = len(case.blk_off) - 1
    v = [0, next(b for b in range(n // 2, -1, -1) if not isinstance(case.tag[b], tuple) and case.tag[b] > c.kCrcChunk), n - 1]
    assert abs(v[1] - n // 2) <= 4
    return v


def check_block_case(case: BlockCase, c=C, shifts=range(16)):
    lens, fr = case.lens(), case.framed()
    single = [i for i, t in enumerate(case.tag) if not isinstance(t, tuple)]
    assert lens[single].tolist() == [case.tag[i] for i in single], "a one-entry block has 18 + klen + vlen bytes"
    assert set(range(19, 300)) <= set(lens.tolist())
    cnt = pc.block_entry_counts(case.blocks, case.blk_off.astype(np.int64))
    many = [i for i, t in enumerate(case.tag) if isinstance(t, tuple)]
    assert cnt[many].tolist() == list(MANY_ENTRIES) and MANY_ENTRIES[0] > 64 >= MANY_ENTRIES[1]
    assert (lens[many] > c.kCrcChunk).all(), "count_block's global path: one pass and a loop of two"
    assert (cnt[single] == 1).all()
    assert all(lens[v] > c.kCrcChunk for v in victims(case, c))
    sets = [kernel_chunks(s + fr.off[:-1], lens, c) for s in shifts]
    return check_chunks(sets, c, "one-entry blocks")


# e. persistent crc_kernel
MAX_PER_CU = 8   # four-wave workgroups that fit a CU at most


def persistent_kernel_nblk(cus):
    return 3 * 4 * MAX_PER_CU * cus + 7


def persistent_kernel_case(cus, seed=505):
    rng = np.random.default_rng(seed)
    specs = [_one_entry(int(L), rng) for L in rng.integers(19, 61, persistent_kernel_nblk(cus))]
    kv, seg = _block_kv(specs, rng)
    return BlockCase(kv, seg, BLOCK_BS).encode()


def check_persistent_kernel(nblk, cus):
    """Every wave takes three blocks or more at any occupancy: the metadata that runs two blocks
    ahead is used at every distance (the block after next exists, is the last, is missing)."""
    lo = []
    for per_cu in range(1, MAX_PER_CU + 1):
        per = kernel_launch(nblk, cus, per_cu)
        assert per.min() >= 3 and per.sum() == nblk, (per_cu, per.min())
        lo.append(int(per.min()))
    assert nblk % 4 == 3
    return f"{nblk} blocks on {cus} CUs: blocks per wave at least {lo} for 1..{MAX_PER_CU} workgroups per CU"


# f. BlockMeta sections of a chosen length
@dataclass
class MetaCase(BlockCase):
    region: list = field(default_factory=list)   # per section, its CRC'd bytes: 32 + a + b


def meta_case(c=C, seed=506):
    """One segment per length, one two-entry block per segment with keys of a <= b bytes: the
    section is 40 + a + b bytes, its CRC'd region section[4:-4] 32 + a + b."""
    rng = np.random.default_rng(seed)
    ls = probe_lengths(34, (1, 2), 80, c)
    ls = [ls[i] for i in rng.permutation(len(ls))]
    specs = [([(n - 32) // 2, (n - 32) - (n - 32) // 2], [0, 0]) for n in ls]
    kv, seg = _block_kv(specs, rng, order=False)
    # the two keys of a segment ascend whatever their lengths
    k0 = kv.key_off[:-1].astype(np.int64)
    kv.keys[k0[0::2]] = rng.integers(1, 0x80, len(ls), dtype=np.uint8)
    kv.keys[k0[1::2]] = rng.integers(0x80, 256, len(ls), dtype=np.uint8)
    case = MetaCase(kv, seg, BLOCK_BS, region=ls).encode()
    return case


def meta_sections(case: MetaCase):
    """pyref's BlockMeta section of every segment."""
    out = []
    for s in range(len(case.seg) - 1):
        k0, _, _ = case.kv.entry(2 * s)
        k1, _, _ = case.kv.entry(2 * s + 1)
        out.append(pyref.encode_block_meta([(0, k0, k1)]))
    return out


def meta_leads(case: MetaCase, meta_addr):
    """Every section's CRC'd region under a section buffer at meta_addr: (addresses, lengths)."""
    sec = np.asarray(case.region, np.int64) + 8
    moff = np.concatenate([[0], np.cumsum(sec)])
    return meta_addr + 4 + moff[:-1], np.asarray(case.region, np.int64)


def check_meta_case(case: MetaCase, c=C, addrs=range(16)):
    assert set(range(34, 301)) <= set(case.region) and [len(s) - 8 for s in meta_sections(case)] == case.region
    cnt = pc.block_entry_counts(case.blocks, case.blk_off.astype(np.int64))
    assert (cnt == 2).all()
    assert {x & 1 for x in case.region} == {0, 1}
    sets = [kernel_chunks(*meta_leads(case, a), c) for a in addrs]
    return check_chunks(sets, c, "BlockMeta sections", section=True)


# ------------------------------------------------------------------------------- sensitivity
def mutants(m: bytes, i: int):
    """m with byte i dropped, duplicated, zeroed."""
    return m[:i] + m[i + 1:], m[:i + 1] + m[i:], m[:i] + b"\0" + m[i + 1:]


def sensitivity(r: Ranges, edges, crc=zlib.crc32):
    """For every block, CRC-32 restated with one byte dropped, duplicated or zeroed at the block's
    first byte, its last, either side of every chunk edge (edges(L) -> block offsets), and with the
    byte just outside either end taken in: each must differ from the block's own CRC.  A zeroed
    byte that was zero already is no mutant; -> [(block, position)] of those."""
    vacuous = []
    for b in range(r.nblk):
        s, e = int(r.off[b]), int(r.off[b + 1]) - r.tail
        m = r.body[s:e].tobytes()
        want = crc(m)
        if s > 0:
            assert crc(r.body[s - 1:e].tobytes()) != want, (b, "byte before")
        if e < len(r.body):
            assert crc(r.body[s:e + 1].tobytes()) != want, (b, "byte after")
        if not m:
            continue
        pos = {0, len(m) - 1}
        for x in edges(len(m)):
            pos |= {x - 1, x}
        for i in sorted(pos):
            for kind, mu in zip(("dropped", "duplicated", "zeroed"), mutants(m, i)):
                if mu == m:
                    vacuous.append((b, i))
                    continue
                assert crc(mu) != want, (b, i, kind)
    return vacuous
