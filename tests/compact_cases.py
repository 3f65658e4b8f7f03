"""Inputs that put compactions on chosen paths of lsmblk_compact.hip -- TEST INFRASTRUCTURE.

The method of path_cases.py and sst_cases.py for the merge, the rules + gather and the SST
rotation; shared by test_compact_cases.py (CPU) and test_gpu_compact_paths.py (GPU):

  constants    kMS, kMTE, kMTT, kBigTE, kTScan, kGTile, kGScan, kCopyB, kGKImg, kGVImg, kRotWin,
               kRotStep, kRotHops, kRotFillMax read out of the kernel source (LSMBLK_* defaults
               resolved); every size below is derived from them
  classifiers  numpy restatements of what picks a path (a merge tile's entries, a gather round's
               staged predicate, rot_levels, the chain's K).  They only ASSERT COVERAGE; expected
               output comes from oracle/ alone.
  generators   run sets and kept streams; each takes the constants it is built for, and the
               check_* functions take the constants they check against, so a case built for other
               constants fails them.
"""
import os
import re
from dataclasses import dataclass, field

import numpy as np

import path_cases as pc
from oracle import oracle as O

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsm_amd", "csrc",
                    "lsmblk_compact.hip")
NAMES = ("kMS", "kMTE", "kMTT", "kBigTE", "kTScan", "kGTile", "kGScan", "kCopyB", "kGKImg", "kGVImg", "kRotWin",
         "kRotStep", "kRotHops", "kRotFillMax")
ROUND = 256  # entries per round of mflag / mwrite / rot_adj / rot_next (their 256 threads, a literal there)


@dataclass(frozen=True)
class Consts:
    kMS: int
    kMTE: int
    kMTT: int
    kBigTE: int
    kTScan: int
    kGTile: int
    kGScan: int
    kCopyB: int
    kGKImg: int
    kGVImg: int
    kRotWin: int
    kRotStep: int
    kRotHops: int
    kRotFillMax: int


def kernel_constants(path=_SRC):
    """The compaction kernels' constants from `path`: `constexpr uintNN_t NAME = N;`, or
    `= LSMBLK_X;` with the `#define LSMBLK_X N` default resolved.  A missing one raises."""
    with open(path) as f:
        text = f.read()
    out = {}
    for name in NAMES:
        m = re.search(r"^\s*constexpr\s+uint(?:32|64)_t\s+%s\s*=\s*(\w+)\s*;" % name, text, re.M)
        if not m:
            raise RuntimeError(f"{name}: no `constexpr uintNN_t {name} = ...;` in {path}")
        v = m.group(1)
        if not v.isdigit():
            d = re.search(r"^#define\s+%s\s+(\d+)\s*$" % v, text, re.M)
            if not d:
                raise RuntimeError(f"{name}: no `#define {v} N` in {path}")
            v = d.group(1)
        out[name] = int(v)
    return Consts(**out)


C = kernel_constants()


@dataclass
class Case:
    kv: O.KV
    rs: np.ndarray                      # u32[nrun + 1]
    info: dict = field(default_factory=dict)

    def runs(self):
        ents = self.kv.entries()
        return [ents[int(a):int(b)] for a, b in zip(self.rs[:-1], self.rs[1:])]


def case_of_runs(runs, **info):
    ents = [e for r in runs for e in r]
    rs = np.zeros(len(runs) + 1, np.uint32)
    rs[1:] = np.cumsum([len(r) for r in runs])
    return Case(O.KV.from_entries(ents), rs, info)


def fixed_kv(kint, klen, vlen, ts, rng):
    """Keys = the low `klen` bytes of kint, big-endian; values random of vlen[i] bytes."""
    n = len(kint)
    keys = np.ascontiguousarray(np.asarray(kint, np.uint64).astype(">u8").view(np.uint8).reshape(n, 8)[:, 8 - klen:])
    vo = np.zeros(n + 1, np.uint32)
    vo[1:] = np.cumsum(vlen)
    return O.KV(keys.reshape(-1), (np.arange(n + 1, dtype=np.uint64) * klen).astype(np.uint32),
                rng.integers(0, 256, int(vo[-1]), dtype=np.uint8), vo, np.asarray(ts, np.uint64))


def prefix_kv(kv, n):
    """The first n entries of kv."""
    return O.KV(kv.keys[:int(kv.key_off[n])], kv.key_off[:n + 1], kv.vals[:int(kv.val_off[n])], kv.val_off[:n + 1],
                kv.ts[:n])


# ------------------------------------------------------------------------------- classifiers
def key_ranks(kv):
    """An order-isomorphic integer per entry's user key."""
    kl = np.diff(kv.key_off.astype(np.int64))
    if kv.n and 0 < kl[0] <= 8 and (kl == kl[0]).all():
        w = int(kl[0])
        a = kv.keys[:kv.n * w].reshape(kv.n, w)
        v = np.zeros(kv.n, np.uint64)
        for j in range(w):
            v = (v << np.uint64(8)) | a[:, j].astype(np.uint64)
        return v
    kb, ko = kv.keys.tobytes(), kv.key_off.tolist()
    keys = [kb[ko[i]:ko[i + 1]] for i in range(kv.n)]
    order = {k: r for r, k in enumerate(sorted(set(keys)))}
    return np.array([order[k] for k in keys], np.uint64)


def tile_totals(kv, rs, c=C, src=None):
    """Entries of every merge tile: the candidates (every kMS-th entry of every run) sorted by (key,
    run, index); tile t = the keys in [candidate t, candidate t + 1) by key-only lower bounds in
    every run.  With src (the oracle's merged input indices) also the tiles' survivor counts."""
    kr, rs = key_ranks(kv), np.asarray(rs, np.int64)
    nrun = len(rs) - 1
    cpos = np.concatenate([np.arange(rs[r], rs[r + 1], c.kMS) for r in range(nrun)])
    crun = np.concatenate([np.full(len(range(int(rs[r]), int(rs[r + 1]), c.kMS)), r) for r in range(nrun)])
    ck = kr[cpos][np.lexsort((cpos, crun, kr[cpos]))]
    total = np.zeros(len(cpos), np.int64)
    surv = np.zeros(len(cpos), np.int64)
    alive = np.zeros(kv.n, bool)
    if src is not None:
        alive[np.asarray(src, np.int64)] = True
    for r in range(nrun):
        run = kr[rs[r]:rs[r + 1]]
        lb = np.concatenate([np.searchsorted(run, ck, "left"), [len(run)]])
        total += np.diff(lb)
        cs = np.concatenate([[0], np.cumsum(alive[rs[r]:rs[r + 1]])])
        surv += np.diff(cs[lb])
    return (total, surv) if src is not None else total


def tile_kernel(total, c=C):
    return "empty" if total == 0 else "tile" if total <= c.kMTE else "big" if total <= c.kBigTE else "global"


def gather_rounds(kl, vl, kept, c=C):
    """Per round of 256 merged positions of mwrite_kernel: kept key / value bytes, the leads
    K0 & 15 / V0 & 15, the staged predicate, and the largest 16-B piece count of one wave."""
    kl, vl, kept = np.asarray(kl, np.int64), np.asarray(vl, np.int64), np.asarray(kept, bool)
    nr = (len(kl) + ROUND - 1) // ROUND
    pad = nr * ROUND - len(kl)
    k = np.pad(np.where(kept, kl, 0), (0, pad)).reshape(nr, ROUND)
    v = np.pad(np.where(kept, vl, 0), (0, pad)).reshape(nr, ROUND)
    kb, vb = k.sum(1), v.sum(1)
    klead, vlead = (np.cumsum(kb) - kb) & 15, (np.cumsum(vb) - vb) & 15
    pieces = lambda x: np.where(x >= 16, (x + 15) >> 4, 0).reshape(nr, ROUND // 64, 64).sum(2).max(1)
    return dict(kb=kb, vb=vb, klead=klead, vlead=vlead, nkept=np.pad(kept, (0, pad)).reshape(nr, ROUND).sum(1),
                staged=(kb + klead <= c.kGKImg) & (vb + vlead <= c.kGVImg),
                k_ok=kb + klead <= c.kGKImg, v_ok=vb + vlead <= c.kGVImg, kpieces=pieces(k), vpieces=pieces(v))


def merged_lengths(kv, src):
    src = np.asarray(src, np.int64)
    return (np.diff(kv.key_off.astype(np.int64))[src], np.diff(kv.val_off.astype(np.int64))[src])


def rot_levels(target, block_size, c=C):
    """rot_levels of lsmblk_compact.hip."""
    j, k = target // 23 + 2, 1
    while k < 32 and (1 << (k - 1)) < j:
        k += 1
    if c.kRotHops and block_size:
        jb, lv = target // block_size // c.kRotHops + 1, 1
        while lv < k and (1 << (lv - 1)) < jb:
            lv += 1
        k = lv
    return k


def rot_double_launches(levels):
    """(rot_double2_kernel, rot_double_kernel) launches of rotation_chains."""
    return (levels - 1) // 2, (levels - 1) % 2


def chain_plan(sst_cap, c=C):
    """rotation_locked's chain: (lc, K or None for doubling to the end, walk + fill launched,
    rot_chain_kernel launches)."""
    lc = 0
    while lc < 32 and (1 << lc) < sst_cap:
        lc += 1
    K = 3 if lc <= 12 else (lc - 9 if lc - 9 <= c.kRotFillMax else None)
    walks = K is not None and (1 << K) < sst_cap
    return lc, K, walks, (K if walks else lc)


def block_counts(kv, seg, bs):
    """Entries of every block of the oracle's encoding of kv's segments."""
    rc, blocks, off = O.encode_segments(kv, np.asarray(seg, np.uint32), bs)
    assert rc == 0
    return pc.block_entry_counts(blocks, off.astype(np.int64))


def block_end(kv, s, bs, span=8192):
    """The greedy end of a block starting at entry s (the oracle's), as rot_next_kernel's J0[s]."""
    rc, blocks, off = O.encode_span(kv, [s, min(kv.n, s + span)], bs)
    assert rc == 0
    return s + int(pc.block_entry_counts(blocks, off.astype(np.int64))[0])


# ------------------------------------------------------------------------------- key order
KEY_ORDER_LAST = (1, 2, 3)  # the arena's last key ends this many bytes past a dword of its tail


def key_order_keys(seed=11):
    P = bytes(range(0x41, 0x51))
    ks = {b"\0" * i for i in range(1, 21)}
    for k in (b"k", b"key", b"fourteen-bytes", b"fifteen--bytes!", P[::-1]):
        ks |= {k, k + b"\0", k + b"\0\0"}
    ks |= {P, P + b"\0", P + b"\1"}
    for d in (1, 2, 3, 4, 5, 8, 9):
        Q, common = bytes([0x60 + d]) * 16, bytes(range(1, d))
        ks.add(Q + common + b"\x40")                       # tail of d bytes
        for extra in range(1, 5):                          # tails of d + 1 .. d + 4, first differing at byte d
            ks.add(Q + common + b"\x41" + b"\x07" * extra)
            ks.add(Q + common + b"\x3f" + b"\xf7" * extra)
    for pos in (0, 3, 4, 15, 16, 17):
        for b in (0x00, 0x7F, 0x80, 0xFF):
            k = bytearray(b"m" * 18)
            k[pos] = b
            ks.add(bytes(k))
    ks |= {b"q" * 65535, b"q" * 300, b"q" * 17, b"q" * 16}
    rng = np.random.default_rng(seed)
    alpha = np.array([0x00, 0x01, 0x7F, 0x80, 0xFF], np.uint8)
    while len(ks) < 300:
        ks.add(bytes(alpha[rng.integers(0, 5, int(rng.integers(1, 25)))]))
    return ks


def key_order(last=1, seed=11):
    """~300 keys that tie on their zero-padded 16-byte images, over 3-5 runs with overlaps and 1-3
    versions; the arena's last key is long and ends `last` bytes past a dword of its tail."""
    rng = np.random.default_rng(seed + last)
    nrun = 3 + last % 3
    lastkey = b"\xff" * 28 + b"\xfe" * last
    runs = [dict() for _ in range(nrun)]
    for k in sorted(key_order_keys(seed)):
        for r in rng.choice(nrun, size=int(rng.integers(1, 4)), replace=False):
            nv = 1 if len(k) > 1000 else int(rng.integers(1, 4))
            tss = sorted(rng.choice(1000, size=nv, replace=False).tolist(), reverse=True)
            runs[int(r)][k] = [(k, int(t) + 1, bytes(rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8)))
                               for t in tss]
    runs[0][lastkey] = [(lastkey, 900, b"first")]
    runs[1][lastkey[:-1]] = [(lastkey[:-1], 800, b"")]
    runs[-1][lastkey] = [(lastkey, 700, b"x"), (lastkey, 100, b"")]
    runs = [[e for k in sorted(r) for e in r[k]] for r in runs]
    assert runs[-1][-1][0] == lastkey and max(k for r in runs for k, _, _ in r) == lastkey
    return case_of_runs(runs, lastkey=lastkey)


def check_key_order(case):
    keys = {k for r in case.runs() for k, _, _ in r}
    assert len(keys) >= 300 and any(len(k) == 65535 for k in keys)
    img = {}
    for k in keys:
        img.setdefault(k[:16].ljust(16, b"\0"), []).append(k)
    ties = [v for v in img.values() if len(v) > 1]
    # 20 zero keys, 5 x 3 zero-extended, P x 3, 7 x 9 tails, 4 x q: keys that share a 16-byte image
    assert sum(len(v) for v in ties) >= 20 + 15 + 3 + 63 + 4
    assert any(min(len(k) for k in v) < 16 and max(len(k) for k in v) > 16 for v in ties)
    assert (len(case.info["lastkey"]) - 16) % 4 in KEY_ORDER_LAST
    assert case.kv.entry(case.kv.n - 1)[0] == case.info["lastkey"]
    return len(keys), len(ties)


def pad_lcp(groups=8):
    """Groups B, B\\0\\0\\1, B\\0\\0\\2, B\\0\\0\\3: the 16-byte images of B and its successor first differ
    two bytes past B's end (zero pad against zero bytes, then against a key byte), so their LCP is
    len(B), not the images' first differing byte.  At 64-byte blocks the true packing is {B, F1},
    {F2, F3} per group; with the longer LCP F2 would still fit the first block, which moves the
    first SST's end at target 1."""
    run = []
    for i in range(groups):
        B = b"pad" + bytes([i + 1]) + b"xy"
        run.append((B, 5, b""))
        run += [(B + b"\0\0" + bytes([j]), 5, b"v" if j == 3 else b"") for j in (1, 2, 3)]
    return case_of_runs([run])


def check_pad_lcp(case):
    assert (block_counts(case.kv, [0, case.kv.n], CHAIN_BS) == 2).all()
    want = O.segment_like_compaction(case.kv, CHAIN_BS, 1)
    assert want[1] == 3   # the first SST ends at the key change after the second block's start
    return len(want) - 1


# ------------------------------------------------------------------------------- tile edges
TILE_NRUN = (1, 2, 3, 64)


def tile_edge_sizes(c=C):
    return (c.kMTE - 1, c.kMTE, c.kMTE + 1, c.kBigTE - 1, c.kBigTE, c.kBigTE + 1, 2 * c.kBigTE + 3)


def _tile_edge_runs(hot, nrun, kMS):
    if nrun == 1:
        shares = [hot]
    elif nrun == 2:
        shares = [hot // 3, hot - hot // 3]
    elif nrun == 3:
        shares = [hot // 2, hot // 3, hot - hot // 2 - hot // 3]
    else:
        shares = [hot // nrun + (1 if r < hot % nrun else 0) for r in range(nrun)]
    if nrun > 1 and shares[-1] % kMS == 0:   # (the trailing key would be a candidate: a tile of its own)
        shares[-1] -= 1
        shares[0] += 1
    H = b"hot-key-of-%d" % hot
    runs = []
    for r, sh in enumerate(shares):
        run = [(b"a-first", 7, b"a")] if r == 0 else []
        run += [(H, 10000 * (nrun - r) + sh - j, b"%d.%d" % (r, j) if j % 5 else b"") for j in range(sh)]
        if nrun > 1 and r == nrun - 1:
            run.append((b"zz-last", 3, b"z"))  # b's last key lies above the hot key (two-level)
        runs.append(run)
    return runs


def tile_edge(X, nrun, c=C):
    """One hot key whose tile holds exactly X entries, in one run (all survive) or split over nrun
    runs (the lowest run's survive); the last run's trailing key counts into the tile unless it
    is a candidate itself."""
    for hot in (X - 1, X) if nrun > 1 else (X,):
        case = case_of_runs(_tile_edge_runs(hot, nrun, c.kMS), X=X, nrun=nrun)
        if tile_totals(case.kv, case.rs, c).max() == X:
            return case
    raise AssertionError(f"no tile of {X} entries over {nrun} runs")


def check_tile_edge(case, c=C):
    """The case's largest tile sits on the side of kMTE / kBigTE it was built for (by its X)."""
    src = O.merge_runs(case.kv, case.rs)
    total, surv = tile_totals(case.kv, case.rs, c, src)
    X = case.info["X"]
    assert X in tile_edge_sizes(c), (X, tile_edge_sizes(c))
    assert total.max() == X and (np.sort(total)[:-1] <= 1).all(), np.sort(total)[-3:]
    if case.info["nrun"] == 1:
        assert surv.max() == X   # every entry survives: sp[] reaches the tile's size
    return tile_kernel(int(total.max()), c), int(surv.max())


# ------------------------------------------------------------------------------- tile scan
def tile_scan_ncs(c=C):
    return (c.kTScan, c.kTScan + 1, 2 * c.kTScan + 2)


def tile_scan(nc, c=C, seed=5):
    """Two runs of distinct 8-byte keys with exactly nc candidates (= tiles): run 1 repeats about
    every 7th key of run 0 (and loses them to it), so the tiles' survivor counts differ."""
    rng = np.random.default_rng(seed)
    n1c = nc // 8
    n0c = nc - n1c
    n0 = n0c * c.kMS if nc == c.kTScan else (n0c - 1) * c.kMS + 1
    n1 = n1c * c.kMS
    k0 = np.arange(n0, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    k1 = k0[np.cumsum(rng.integers(1, 13, n1)) - 1]   # gaps of 1..12: run 1's candidates cut run 0's tiles unevenly
    assert n0 > 12 * n1 // 2 + 6 * int(np.sqrt(n1)) + 12
    kint = np.concatenate([k0, k1])
    vlen = (np.arange(n0 + n1) * 7 // 3) % 4
    ts = np.concatenate([np.full(n0, 2), np.full(n1, 1)])
    return Case(fixed_kv(kint, 8, vlen, ts, rng), np.array([0, n0, n0 + n1], np.uint32), dict(nc=nc))


def check_tile_scan(case, c=C):
    total, surv = tile_totals(case.kv, case.rs, c, O.merge_runs(case.kv, case.rs))
    nc = len(total)
    assert nc == case.info["nc"] and nc in tile_scan_ncs(c), (nc, tile_scan_ncs(c))
    parts = (nc + c.kTScan - 1) // c.kTScan
    assert len(set(surv.tolist())) > 3 and total.max() <= c.kMTE
    return nc, parts


# ------------------------------------------------------------------------------- gather scan
def gather_scan(c=C, seed=6):
    """kGScan * kGTile + kGTile + 5 merged entries (a second scan part of two tiles): two versions
    per key around the watermark, tombstones, one prefix; 8-byte keys, values of 0-2 bytes."""
    rng = np.random.default_rng(seed)
    M = c.kGScan * c.kGTile + c.kGTile + 5
    nk = (M + 1) // 2
    kid = np.repeat(np.arange(nk, dtype=np.uint64), 2)[:M]
    ver = (np.arange(M) % 2)
    cls = np.repeat(rng.integers(0, 4, nk), 2)[:M]   # above/below, below/below, above/above, tombstone
    wm = 1000
    above = (cls == 2) | ((cls == 0) & (ver == 0))
    ts = np.where(above, 2000 - ver, 500 - ver)
    vlen = rng.integers(0, 3, M)
    vlen[(cls == 3) & (ver == 0)] = 0
    k0 = kid * np.uint64(2) + np.uint64(1)
    n1 = nk // 5
    k1 = k0[::2][np.arange(n1) * 5]
    kint = np.concatenate([k0, k1])
    kv = fixed_kv(kint, 8, np.concatenate([vlen, np.full(n1, 1)]), np.concatenate([ts, np.full(n1, 1)]), rng)
    prefix = int(k0[M // 2 + 12345]).to_bytes(8, "big")[:6]
    return Case(kv, np.array([0, M, M + n1], np.uint32), dict(M=M, wm=wm, prefix=prefix))


def check_gather_scan(case, kept, c=C):
    """kept: the oracle's kept merged positions."""
    M = case.info["M"]
    tiles = (M + c.kGTile - 1) // c.kGTile
    assert tiles == c.kGScan + 2, (tiles, c.kGScan)
    flag = np.zeros(M, bool)
    flag[kept] = True
    per = np.add.reduceat(flag, np.arange(0, M, c.kGTile))
    assert len(set(per.tolist())) > 10 and 0 < len(kept) < M
    return tiles, (tiles + c.kGScan - 1) // c.kGScan, int(per[:c.kGScan].sum())


# ------------------------------------------------------------------------------- round straddle
STRADDLE_SIZES = (2, 3, 5)


def round_straddle(c=C, wm=1000):
    """Version groups of 2, 3 and 5 entries that end at, start at and span the merged positions
    256 m and kGTile m, timestamps on both sides of the watermark, some first entries tombstones.
    Run 1 holds only keys above run 0's, so merged position = input position in both modes."""
    want = {}
    for j in range(1, 13 * c.kGTile // ROUND + 1):
        P = j * ROUND
        if (j * ROUND // c.kGTile + j) % 2 == 0:
            g = STRADDLE_SIZES[j % 3]
            want[P - g] = g                                  # ends at P
            want[P] = STRADDLE_SIZES[(j + 1) % 3]            # starts at P
        else:
            g = STRADDLE_SIZES[j % 3]
            want[P - 1 - (j // 2) % (g - 1)] = g             # spans P
    run, kid, q, nspan = [], 0, 0, {False: 0, True: 0}
    end = max(want) + 40
    while len(run) < end:
        pos = len(run)
        g = want.get(pos, 1)
        assert all(p <= pos or p >= pos + g for p in want), (pos, g)
        key = kid.to_bytes(4, "big") + b"k"
        kid += 1
        if g == 1:
            run.append((key, wm + 5 if pos % 3 else wm - 5, b"" if pos % 7 == 0 else b"v%d" % (pos % 10)))
            continue
        above = q % (g + 1)
        P = (pos + g - 1) // ROUND * ROUND
        if pos < P:   # spans P: predecessor / entry at P above-above, above-below, below-below in turn
            big = P % c.kGTile == 0
            above = (P - pos + 1, P - pos, 0)[nspan[big] % 3]
            nspan[big] += 1
        for i in range(g):
            run.append((key, wm + g - i if i < above else wm - i, b"" if (i == 0 and q % 3 == 0) else b"g%d" % i))
        q += 1
    tail = [((kid + 5 + i // 2).to_bytes(4, "big") + b"k", 9 - i % 2, b"b") for i in range(6)]
    return case_of_runs([run, tail], wm=wm, prefix=b"\0\0", n0=len(run))   # (every key: a prefix-filtered entry at every multiple)


def check_round_straddle(case, c=C):
    """Which kinds of group meet which multiples: {(multiple of kGTile?, kind, predecessor at or
    below the watermark, entry at or below)}."""
    src = O.merge_runs(case.kv, case.rs).astype(np.int64)
    kr, ts, wm = key_ranks(case.kv)[src], case.kv.ts[src].astype(np.int64), case.info["wm"]
    assert (src[:case.info["n0"]] == np.arange(case.info["n0"])).all()
    seen = set()
    for P in range(ROUND, case.info["n0"] - 8, ROUND):
        big = P % c.kGTile == 0
        if kr[P - 1] == kr[P]:
            seen.add((big, "span", bool(ts[P - 1] <= wm), bool(ts[P] <= wm)))
        else:
            if kr[P - 2] == kr[P - 1]:
                seen.add((big, "end"))
            if kr[P] == kr[P + 1]:
                seen.add((big, "start"))
    for big in (False, True):
        assert {(big, "end"), (big, "start"), (big, "span", True, True), (big, "span", False, True),
                (big, "span", False, False)} <= seen, (big, sorted(seen, key=str))
    assert case.info["n0"] > 6 * c.kGTile
    return seen


# ------------------------------------------------------------------------------- copy shapes
LENS = (1, 3, 4, 7, 8, 15, 16, 17, 31, 32, 128, 129, 130, 257, 1000)
_SMALL, _BIG = LENS[:10], LENS[10:]


def _lens_for_sum(T, count, rot, minlen, big_every, ones=6):
    """`count` lengths of LENS (and minlen; at most `ones` of length 1, which a key can take only
    where its first byte changes) that sum to exactly T, cycling through LENS."""
    small = _SMALL if minlen else (0,) + _SMALL
    out, S = [], 0
    for i in range(count):
        want = _BIG[(i // big_every + rot) % len(_BIG)] if i % big_every == 5 else small[(i + rot) % len(small)]
        if want == 1 and minlen > 1:
            ones -= 1
            want = 1 if ones >= 0 else minlen
        left = count - i - 1
        ln = want if S + want + left * minlen <= T else minlen
        out.append(ln)
        S += ln
    assert S <= T, (S, T)
    opts = sorted(set(LENS) | {minlen})
    keep = min(32, count // 2)   # the first entries keep the cycle's lengths
    while S < T:
        best = None
        for lo in (keep, 0):
            for i in range(lo, count):
                for ln in opts:
                    if out[i] != 1 and out[i] < ln and ln - out[i] <= T - S and (best is None or ln - out[i] > best[0]):
                        best = (ln - out[i], i, ln)
            if best:
                break
        assert best, (S, T)
        out[best[1]] = best[2]
        S += best[0]
    return out


def copy_shape(c=C, nlead=16, wm=100, seed=8):
    """A one-run stream (merged position = input position) of rounds of 256 entries whose key and
    value lengths cycle over LENS (values: and 0), shaped per round (info["rounds"]):
      lead      all kept; key bytes = 1 and value bytes = 3 (mod 16), so the leads take every value
      kimg      kept key bytes + lead == kGKImg (staged)      kimg+1   one more (unstaged by keys alone)
      vimg      kept value bytes + lead == kGVImg (staged)    vimg+1   one more (unstaged by values alone)
      pieces    staged, wave 0 holds more than 64 * kCopyB 16-byte value pieces
      mixed     kept and dropped entries interleaved (version groups below the watermark)
    and a last round partly filled."""
    rng = np.random.default_rng(seed)
    ents, rounds, st = [], [], dict(cnt=0, K=0, V=0)

    def next_key(klen):
        # keys ascend whatever their lengths: a 3-byte counter, then random bytes; a 1-byte key
        # opens a new first byte
        if klen == 1:
            st["cnt"] = (st["cnt"] | 0xFFFF) + 1
            return bytes([st["cnt"] >> 16])
        st["cnt"] += 1
        return st["cnt"].to_bytes(3, "big") + bytes(rng.integers(0, 256, klen - 3, dtype=np.uint8))

    def emit(tag, kls, vls, groups=None):
        groups = groups or [1] * len(kls)
        assert sum(groups) == ROUND or tag == "tail"
        for kl, vl, g in zip(kls, vls, groups):
            key = next_key(kl)
            for i in range(g):
                v = bytes(rng.integers(0, 256, vl, dtype=np.uint8))
                ents.append((key, (wm + 50 if g == 1 else wm - 1 - i), v))
            st["K"] += kl
            st["V"] += vl
        rounds.append(tag)

    def resid(T, want):  # the largest value <= T that is `want` mod 16
        return T - (T - want) % 16

    for r in range(nlead):
        emit("lead", _lens_for_sum(resid(2600, 1), ROUND, r, 3, 32), _lens_for_sum(resid(9000, 3), ROUND, r + 3, 0, 16))
    emit("kimg", _lens_for_sum(c.kGKImg - (st["K"] & 15), ROUND, 1, 3, 32), _lens_for_sum(5003, ROUND, 2, 0, 16))
    emit("kimg+1", _lens_for_sum(c.kGKImg + 1 - (st["K"] & 15), ROUND, 3, 3, 32), _lens_for_sum(5005, ROUND, 4, 0, 16))
    emit("vimg", _lens_for_sum(3001, ROUND, 5, 3, 32), _lens_for_sum(c.kGVImg - (st["V"] & 15), ROUND, 6, 0, 16))
    emit("vimg+1", _lens_for_sum(3003, ROUND, 7, 3, 32), _lens_for_sum(c.kGVImg + 1 - (st["V"] & 15), ROUND, 8, 0, 16))
    np16 = 64 * c.kCopyB + 9   # 16-B pieces of wave 0's values
    wave0 = [1000] * (np16 // 63) + [16 * (np16 % 63) - 3] + [0] * 64
    emit("pieces", _lens_for_sum(2005, ROUND, 9, 3, 32), wave0[:64] + _lens_for_sum(4001, ROUND - 64, 10, 0, 16))
    for r, vsum in ((0, 6007), (1, 7001)):
        groups = []
        while sum(groups) < ROUND:
            groups.append(min((2, 1, 3, 1, 1, 2)[len(groups) % 6], ROUND - sum(groups)))
        emit("mixed", _lens_for_sum(1501 + r, len(groups), 11 + r, 3, 32),
             _lens_for_sum(vsum, len(groups), 12 + r, 0, 16), groups)
    groups = [(3, 1, 2, 1)[i % 4] for i in range(200)]
    groups = groups[:next(i for i in range(200) if sum(groups[:i + 1]) >= ROUND)]
    groups.append(ROUND - sum(groups))
    emit("mixed-unstaged", _lens_for_sum(c.kGKImg + 500, len(groups), 13, 3, 32),
         _lens_for_sum(c.kGVImg + 700, len(groups), 14, 0, 16), groups)
    emit("tail", _lens_for_sum(700, 37, 15, 3, 32), _lens_for_sum(900, 37, 16, 0, 16))
    return case_of_runs([ents], wm=wm, rounds=rounds)


def check_copy_shape(case, kept, c=C, nlead=16):
    """kept: the oracle's kept merged positions under the case's watermark (no prefix, not bottom)."""
    kl, vl = merged_lengths(case.kv, np.arange(case.kv.n))
    flag = np.zeros(case.kv.n, bool)
    flag[kept] = True
    g, tags = gather_rounds(kl, vl, flag, c), case.info["rounds"]
    assert len(tags) == len(g["kb"])
    at = lambda t: [i for i, x in enumerate(tags) if x == t]
    for i in at("lead"):
        assert g["staged"][i] and g["nkept"][i] == ROUND
    if nlead >= 16:
        assert set(g["klead"][g["staged"]].tolist()) == set(range(16)) == set(g["vlead"][g["staged"]].tolist())
    (a,), (b,), (d,), (e,), (p,) = at("kimg"), at("kimg+1"), at("vimg"), at("vimg+1"), at("pieces")
    assert g["kb"][a] + g["klead"][a] == c.kGKImg and g["staged"][a]
    assert g["kb"][b] + g["klead"][b] == c.kGKImg + 1 and g["v_ok"][b] and not g["staged"][b]
    assert g["vb"][d] + g["vlead"][d] == c.kGVImg and g["staged"][d]
    assert g["vb"][e] + g["vlead"][e] == c.kGVImg + 1 and g["k_ok"][e] and not g["staged"][e]
    assert g["staged"][p] and g["vpieces"][p] > 64 * c.kCopyB
    for i in at("mixed"):
        assert g["staged"][i] and ROUND // 2 < g["nkept"][i] < ROUND
    (u,) = at("mixed-unstaged")
    assert not g["staged"][u] and g["nkept"][u] < ROUND
    assert 0 < g["nkept"][-1] < ROUND
    for ln, name in ((kl, "key"), (vl, "value")):   # every length of LENS, staged and unstaged
        for staged in (True, False):
            rows = np.repeat(g["staged"] == staged, ROUND)[:len(ln)] & flag
            assert set(LENS) <= set(ln[rows].tolist()), (name, staged, sorted(set(LENS) - set(ln[rows].tolist())))
    assert 0 in vl[flag]
    return g


def copy_coverage(g):
    s = g["staged"]
    return (f"copy-shape: {len(s)} rounds, {int(s.sum())} staged (key leads {sorted(set(g['klead'][s].tolist()))}, "
            f"value leads {sorted(set(g['vlead'][s].tolist()))}), unstaged by keys {int((~g['k_ok'] & g['v_ok']).sum())}, "
            f"by values {int((g['k_ok'] & ~g['v_ok']).sum())}, by both {int((~g['k_ok'] & ~g['v_ok']).sum())}; "
            f"max key bytes + lead {int((g['kb'] + g['klead'])[s].max())}, value {int((g['vb'] + g['vlead'])[s].max())}; "
            f"most 16-B value pieces in a wave {int(g['vpieces'][s].max())}")


# ------------------------------------------------------------------------------- rotation window
def rot_short_keys(seed=9, nkeys=9000):
    """A sorted stream of 1-2-byte keys (1-2 versions) with empty values: ~17-byte entries, so a
    16 KiB block holds ~950 of them and a 64 KiB block ~3 800 -- every walk leaves the window."""
    rng = np.random.default_rng(seed)
    allk = sorted([bytes([a]) for a in range(256)] + [bytes([a, b]) for a in range(256) for b in range(256)])
    pick = sorted(rng.choice(len(allk), nkeys, replace=False))
    ents = []
    for i in pick:
        nv = 1 + int(rng.integers(0, 2))
        ents += [(allk[i], nv - v, b"") for v in range(nv)]
    return O.KV.from_entries(ents)


def rot_uniform(n=4000, vlen=10, seed=10):
    """Sorted 4-byte keys with vlen-byte values: a 16 KiB block holds ~600 entries, so the block
    ends of a workgroup's 256 starts sweep the window's edge 256 + kRotWin."""
    rng = np.random.default_rng(seed)
    return fixed_kv(np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(77), 4, np.full(n, vlen),
                    np.full(n, 5), rng)


def rot_prefix_runs(n=9000, every=1000, seed=13):
    """Sorted 6-byte keys whose first four bytes change every `every` entries (LCP 0 there, >= 4
    elsewhere) with empty values: ~18-byte entries, and a walk that starts in a workgroup's first
    entries meets the LCP drop only in global memory, past its window."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.uint64)
    kint = ((i // np.uint64(every) + np.uint64(0x10)) * np.uint64(0x01010101) << np.uint64(16)) | (i % np.uint64(every))
    return fixed_kv(kint, 6, np.zeros(n, np.int64), np.full(n, 5), rng)


def check_prefix_runs(kv, bs, c=C, every=1000):
    """A start whose block crosses a prefix change that lies past its workgroup's window."""
    assert every >= ROUND + c.kRotWin
    for s in range(0, ROUND):
        if block_end(kv, s, bs) > every + 1:
            return s
    raise AssertionError("no walk of workgroup 0 crosses the prefix change")


def swap_pair(kv, q):
    """kv with entries q and q + 1 exchanged (their keys differ): one unsorted pair."""
    ents = kv.entries()
    while ents[q][0] == ents[q + 1][0]:
        q += 1
    ents[q], ents[q + 1] = ents[q + 1], ents[q]
    return O.KV.from_entries(ents), q


def window_edge_offsets(c=C):
    return range(ROUND + c.kRotWin - c.kRotStep - 1, ROUND + c.kRotWin + 2)


def check_window_edge(kv, bs, c=C, group=1):
    """Starts of workgroup `group` whose blocks end at every window offset of window_edge_offsets."""
    s0, found = group * ROUND, {}
    guess = block_end(kv, s0, bs) - s0
    for x in window_edge_offsets(c):
        t = x - guess
        for _ in range(6):
            assert 0 <= t < ROUND, (x, t, guess)
            m = block_end(kv, s0 + t, bs) - (s0 + t)
            if t + m == x:
                found[x] = s0 + t
                break
            t = x - m
    assert set(found) == set(window_edge_offsets(c)), (sorted(found), guess)
    return found


def level_targets(bs, c=C):
    """{levels: a target SST size that gives rot_levels(target, bs) == levels}, levels 1..5."""
    out = {1: 4 * bs}
    for lv in range(2, 6):
        out[lv] = (1 << (lv - 2)) * c.kRotHops * bs
    return out


def rot_tiny(n=12):
    """The first n entries of rot_uniform: at block_size 256 (9 entries per block) two blocks, so
    every chain is at the end after one doubling."""
    return prefix_kv(rot_uniform(), n)


def check_levels_not_needed(kv, bs, target, c=C):
    """More levels allocated than needed: some block chain is short of the end after level 0
    (need[0] is set, level 1 runs), none after level 1 -- J0[J0[s]] == n for every s -- so need[1]
    and every flag above stay 0 and the doubling kernels of levels >= 2 return at once."""
    n = kv.n
    J0 = np.array([block_end(kv, s, bs) for s in range(n)] + [n])
    assert rot_levels(target, bs, c) >= 4 and (J0[:n] < n).any() and (J0[J0] == n).all(), J0
    assert len(O.segment_like_compaction(kv, bs, target)) == 2   # one SST
    return rot_levels(target, bs, c)


def check_level_targets(t, bs, c=C):
    for lv, target in t.items():
        assert rot_levels(target, bs, c) == lv, (lv, target, rot_levels(target, bs, c))
    assert t[1] < c.kRotHops * bs


# ------------------------------------------------------------------------------- SST chain
CHAIN_BS = 64


def chain_lcs(c=C):
    """ceil(log2 sst_cap) of the chain cases: K = 3 without and with the walk (3, 4), K = 3 at its
    last lc (12), K = lc - 9 = 4, 5, kRotFillMax - 1, kRotFillMax, and doubling to the end."""
    return (3, 4, 12, 13, 14, 8 + c.kRotFillMax, 9 + c.kRotFillMax, 10 + c.kRotFillMax)


def chain_stream(n, versions=1, seed=12):
    """8-byte keys (`versions` entries each) with 9-byte values: at 64-byte blocks every entry is
    its own block, and at target 1 an SST ends at the first key change after its second entry."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    return fixed_kv((i // versions).astype(np.uint64) * np.uint64(5) + np.uint64(3), 8, np.full(n, 9),
                    versions - i % versions, rng)


def chain_cases(c=C):
    """[(entries, sst_cap, the SST count)]: per lc of chain_lcs a chain of 3 * 2^(lc-2) SSTs that
    fills the array exactly (sst_cap = nsst + 1) and one slot short (LSMBLK_E_CAPACITY), the
    capacities 2^3 and 2^3 + 1 on both sides of the last doubling level's (2 << k) < sst_cap, and
    power-of-two capacities that the doubling levels alone fill."""
    out = []
    for lc in chain_lcs(c):
        nsst = 3 << (lc - 2)
        out += [(2 * nsst, nsst + 1, nsst), (2 * nsst, nsst, nsst)]
    out += [(14, 8, 7), (16, 9, 8), (16, 8, 8), (10, 8, 5), (10, 9, 5), (18, 9, 9)]
    # an array of exactly 2^lc slots with no walk after the doubling (lc <= 3, lc > 9 + kRotFillMax):
    # the last level's elements end at the array's last slot
    top = 10 + c.kRotFillMax
    out += [(2, 2, 1), (4, 2, 2), (6, 4, 3), (8, 4, 4), (2 << top, 1 << top, 1 << top), ((2 << top) - 2, 1 << top, (1 << top) - 1)]
    return out


def check_chain_cases(cases, c=C):
    ks = set()
    for n, cap, nsst in cases:
        lc, K, walks, _ = chain_plan(cap, c)
        ks.add((lc, K, walks, cap > nsst))
    # K = 3 without and with the walk, every step of K = lc - 9 at both ends of its range, doubling
    want = {(3, False), (3, True), (4, True), (5, True), (c.kRotFillMax - 1, True), (c.kRotFillMax, True), (None, False)}
    for fits in (True, False):
        assert want <= {(K, walks) for _, K, walks, ok in ks if ok == fits}, (fits, sorted(ks, key=str))
    return ks
