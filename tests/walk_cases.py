"""Inputs that put the encode plan walk on chosen routes -- TEST INFRASTRUCTURE.

The plan walk (lsm_amd/csrc/lsmblk_gpu.hip: the helper waves plan_produce / plan_produce_pipe, the
walker walk_segment, hosted by plan_walk_kernel and by fuse_walk) decides where every block ends and
which prefix every entry gets.  Shared by test_walk_cases.py (CPU) and test_gpu_walk.py (GPU):

  constants    kRing, kChunk, kProdBatch, kPipeB, kAlcpLcp and the literals of walk_segment's
               narrow / 64-bit split, read out of the kernel source
  classify_pairs   per adjacent pair of keys inside a segment, what the helper computes (min length,
               LCP, order) and the route it takes to it (16-byte select, dword loop, key_diff tail)
  walk         a lane-level restatement of walk_segment over those pair values: 64-entry windows,
               ballot and first stop, the inner loop, the open carry, direct mode, the huge-entry
               restart, u32 against 64-bit arithmetic.  Its block table must equal the oracle's on
               every case; then what it reports about lanes, windows and ring slots can be trusted.
  generators   pair_probes, tail_probes, geometry, direct_rewrap, fused_multi, wide, huge

The classifier and the restatement only ASSERT COVERAGE.  Expected bytes come from the oracle.
Every generator returns (kv, seg_start, block_size), or a list of such cases.
"""
import re
from dataclasses import dataclass, field

import numpy as np

import path_cases as pc
from lsm_amd import synth
from oracle import oracle as O

_SRC = pc._SRC
_NAMES = ("kRing", "kChunk", "kProdBatch", "kPipeB", "kAlcpLcp")


def walk_constants(path=_SRC):
    """The ring / hand-off constants, and from walk_segment's own lines: kHugeRec (a window holding
    r >= it takes the 64-bit path), kNarrowBs (block sizes below it may take the u32 path) and
    kGrowMax (a growth >= it makes the inner loop restart the walk)."""
    K = pc.read_constants(path, _NAMES)
    with open(path) as f:
        text = f.read()
    m = re.search(r"void walk_segment\(.*?^}$", text, re.S | re.M)
    if not m:
        raise RuntimeError(f"walk_segment: not found in {path}")
    body = m.group(0)
    for name, pat, val in (
            ("kNarrowBs", r"narrow\s*=\s*bs\s*<\s*\(1ull\s*<<\s*(\d+)\)", lambda g: 1 << int(g[0])),
            ("kHugeRec", r"r\s*>=\s*\(1u\s*<<\s*(\d+)\)\s*-\s*(\d+)\)", lambda g: (1 << int(g[0])) - int(g[1])),
            ("kGrowMax", r"__ballot\(g2\s*>=\s*\(1u\s*<<\s*(\d+)\)\)", lambda g: 1 << int(g[0]))):
        mm = re.search(pat, body)
        if not mm:
            raise RuntimeError(f"{name}: its line is not in walk_segment ({path})")
        K[name] = val(mm.groups())
    return K


K = walk_constants()
kRing, kChunk, kProdBatch, kPipeB, kAlcpLcp = (K[n] for n in _NAMES)
kPipeE = 64 * kPipeB
kNarrowBs, kHugeRec, kGrowMax = K["kNarrowBs"], K["kHugeRec"], K["kGrowMax"]
UNSORTED = 1 << 31
M32 = (1 << 32) - 1

ROUTES = ("select", "dword", "tail")


# ------------------------------------------------------------------------------- pair classifier
@dataclass
class Pairs:
    """Per adjacent pair (e - 1, e), e = 1 .. n - 1 (index e - 1 in every array)."""
    inside: np.ndarray   # the pair lies inside a segment (e is no segment's first entry)
    m: np.ndarray        # min(pl, kl)
    z: np.ndarray        # the true LCP
    route: np.ndarray    # index into ROUTES
    sorted: np.ndarray   # key[e - 1] <= key[e]
    b0: np.ndarray       # the deciding bytes key[e - 1][z], key[e][z] (0 where z == m)
    b1: np.ndarray
    lead_p: np.ndarray   # (glead + pp) & 15, (glead + kp) & 15: the alignment of the helper's loads
    lead_k: np.ndarray
    glead: int

    @property
    def alcp(self):
        """What the helper hands the walker per entry e (n values; entry 0: 0)."""
        a = np.minimum(self.z, kAlcpLcp) | np.where(self.sorted, 0, UNSORTED)
        return np.concatenate([[0], a]).astype(np.int64)

    def seen(self):
        """{(route, sorted, z & 3)} over the pairs inside segments."""
        i = self.inside
        return set(zip((ROUTES[r] for r in self.route[i]), self.sorted[i].tolist(), (self.z[i] & 3).tolist()))


def classify_pairs(kv, seg, key_addr=0):
    """Pairs of the stream.  key_addr: the key arena's address (its low 4 bits are the helper's glead)."""
    n = kv.n
    ko = kv.key_off.astype(np.int64)
    glead = int(key_addr) & 15
    if n < 2:
        z = np.zeros(0, np.int64)
        return Pairs(z.astype(bool), z, z, z, z.astype(bool), z, z, z, z, glead)
    kl = np.diff(ko)
    pp, kp, pl, kk = ko[:-2], ko[1:-1], kl[:-1], kl[1:]
    m = np.minimum(pl, kk)
    z = np.zeros(n - 1, np.int64)
    act = np.arange(n - 1)
    c = 0
    while act.size:  # byte column c of every pair still equal up to it
        act = act[m[act] > c]
        act = act[kv.keys[pp[act] + c] == kv.keys[kp[act] + c]]
        z[act] = c + 1
        c += 1
    diff = z < m
    b0, b1 = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64)
    b0[diff] = kv.keys[pp[diff] + z[diff]]
    b1[diff] = kv.keys[kp[diff] + z[diff]]
    srt = np.where(diff, b0 < b1, pl <= kk)
    klim = glead + int(ko[-1])
    tail = (glead + kp + 16 > klim) | (glead + pp + 16 > klim)
    route = np.where(tail, 2, np.where((z < 16) | (m <= 16), 0, 1))
    inside = np.ones(n - 1, bool)
    s = np.asarray(seg, np.int64)
    s = s[(s >= 1) & (s <= n - 1)]
    inside[s - 1] = False
    return Pairs(inside, m, z, route, srt, b0, b1, (glead + pp) & 15, (glead + kp) & 15, glead)


def key_of(kv, e):
    return bytes(kv.keys[int(kv.key_off[e]):int(kv.key_off[e + 1])])


def lcp(a, b):
    n = min(len(a), len(b))
    i = 0
    while i < n and a[i] == b[i]:
        i += 1
    return i


def shortcut_differs(kv, P: Pairs, s0, s1):
    """Entries of the one-block run [s0, s1) whose prefix by the walker's min shortcut (the running
    min of the adjacent LCPs) is not their true prefix, the LCP with key s0."""
    k0, run, out = key_of(kv, s0), kAlcpLcp, []
    for e in range(s0 + 1, s1):
        run = min(run, int(P.z[e - 1]))
        if run != lcp(k0, key_of(kv, e)):
            out.append(e)
    return out


def pairs_line(name, P: Pairs):
    seen = P.seen()
    per = {r: sum(1 for x in seen if x[0] == r) for r in ROUTES}
    return (f"{name}: {int(P.inside.sum())} pairs at glead {P.glead}; (route, sorted, z&3) combinations {per}; "
            f"unsorted {int((~P.sorted & P.inside).sum())}; z {int(P.z.min()) if P.z.size else '-'}.."
            f"{int(P.z.max()) if P.z.size else '-'}")


# ------------------------------------------------------------------------------- walk restatement
@dataclass
class Blk:
    seg: int
    first: int
    lane0: int                 # lane of the first entry in the window where the block starts
    inner_opened: bool         # started in the inner loop (on lane f of a window), not at a window's lane 0
    end: int = 0
    size: int = 0
    f: int = -1                # lane of the stop that ended it
    windows: int = 0
    found: str = ""            # the stop came from the 'outer' path or the 'inner' loop
    ended: str = ""            # 'outer' / 'inner' stop at an entry, or the 'segment' end
    carried: tuple = ()        # per window it stayed open across: 'outer' (carry += incl_all) / 'inner' (open)
    direct: bool = False
    direct_window: int = -1    # the block's window (0-based) in which direct mode came on
    slot_first: int = 0
    slot_last: int = 0
    straddle: bool = False     # a window of the block holds ring slots kRing - 1 and 0
    wide: list = field(default_factory=list)  # per window: the 64-bit path ran
    pmin_used: bool = False    # in a later window the carried min is below the window's own running min
    mask_used: bool = False    # inner-opened: a lane <= f holds a smaller alcp than the min over (f, lane]

    @property
    def n(self):
        return self.end - self.first


class Walk:
    """walk_segment over (rec, alcp) per entry, lane by lane.  ring_base[g]: the entry at ring slot 0
    for segment g (plan_walk_kernel: the segment's first; fuse_walk: the walker's first segment's)."""

    def __init__(self, kv, seg, block_size, ring_base=None, pairs=None):
        self.kv, self.bs = kv, int(block_size)
        self.seg = np.asarray(seg, np.int64)
        P = pairs if pairs is not None else classify_pairs(kv, seg)
        self.alcp = P.alcp
        self.rec = (np.diff(kv.key_off.astype(np.int64)) + np.diff(kv.val_off.astype(np.int64)))
        self.blocks, self.edges, self.straddles = [], set(), []
        self.huge_restarts = self.scan64 = self.narrow_near_huge = 0
        base = self.seg[:-1] if ring_base is None else np.asarray(ring_base, np.int64)
        for g in range(len(self.seg) - 1):
            self._segment(g, int(self.seg[g]), int(self.seg[g + 1]), int(base[g]))

    # -- the table the oracle must agree with
    def table(self):
        return (np.array([b.first for b in self.blocks], np.int64), np.array([b.size for b in self.blocks], np.int64))

    def _open(self, g, s, lane0, S0, inner):
        b = Blk(g, s, lane0, inner, slot_first=(s - S0) & (kRing - 1))
        self.blocks.append(b)
        return b

    def _window(self, b, j0, wend, S0):
        b.windows += 1
        if ((j0 - S0) & (kRing - 1)) + (wend - j0) > kRing:
            b.straddle = True
            self.straddles.append((b.seg, j0, b.windows - 1))

    def _close(self, b, end, f, size, found, s1, S0):
        b.end, b.f, b.size, b.found = end, f, int(size) & M32, found
        b.ended = "segment" if end == s1 else found
        b.slot_last = (end - 1 - S0) & (kRing - 1)

    def _direct_lcp(self, s, e):
        return lcp(key_of(self.kv, s), key_of(self.kv, e))

    def _segment(self, g, s0, s1, S0):
        rec, alcp, bs = self.rec, self.alcp, self.bs
        narrow = bs < kNarrowBs
        L = np.arange(64)
        s = s0
        while s < s1:
            carry, pmin, direct = 2, kAlcpLcp, False
            cur = self._open(g, s, 0, S0, False)
            j0 = s
            while True:
                wend = min(s1, j0 + 64)
                e = j0 + L
                valid = e < s1
                ec = np.minimum(e, s1 - 1)
                r = np.where(valid, rec[ec], 0)
                al = np.where(valid & (e != s), alcp[ec], kAlcpLcp)
                self._window(cur, j0, wend, S0)
                if not direct and (al & UNSORTED).any():
                    direct, cur.direct, cur.direct_window = True, True, cur.windows - 1
                a31 = al & kAlcpLcp
                loc = np.minimum.accumulate(a31)
                pmin_in = pmin
                if not direct:
                    p = np.minimum(pmin, loc)
                    pmin = int(p[63])
                else:
                    p = np.zeros(64, np.int64)
                    for l in np.flatnonzero(valid & (e != s)):
                        p[l] = self._direct_lcp(s, int(e[l]))
                p = np.where(e == s, 0, p)
                wide = not (narrow and not (valid & (r >= kHugeRec)).any())
                if not wide:
                    if (valid & (r == kHugeRec - 1)).any():
                        self.narrow_near_huge += 1
                    g32 = np.where(valid, (r + 16 - p) & M32, 0)
                    i32 = np.cumsum(g32) & M32
                    before = ((carry & M32) + i32 - g32) & M32
                    lhs = (before + r + 14) & M32
                    stop = ~valid | ((e != s) & (lhs > (bs & M32)))
                    incl_all = int(i32[63])
                else:
                    gr = np.where(valid, r + 16 - p, 0)
                    incl = np.cumsum(gr)
                    if (gr < kGrowMax).all():
                        incl &= M32
                    else:
                        self.scan64 += 1
                    before = carry + incl - gr
                    lhs = before + r + 14
                    stop = ~valid | ((e != s) & (lhs > bs))
                    incl_all = int(incl[63])
                cur.wide.append(wide)
                path = "wide" if wide else "narrow"
                f = int(np.argmax(stop)) if stop.any() else 64
                mine = (L < f) & (e != s)
                if (mine & (lhs == bs)).any():
                    self.edges.add((path, "eq"))
                if cur.windows > 1 and not direct and (mine & (pmin_in < loc)).any():
                    cur.pmin_used = True
                if f == 64:
                    carry += incl_all
                    cur.carried += ("outer",)
                    j0 += 64
                    continue
                if valid[f] and lhs[f] == bs + 1:
                    self.edges.add((path, "plus1"))
                self._close(cur, j0 + f, f, before[f], "outer", s1, S0)
                s = j0 + f
                opened = False
                while not direct and s < s1:
                    mn = np.minimum.accumulate(np.where(L <= f, kAlcpLcp, a31))
                    p2 = np.where(L <= f, 0, mn)
                    g2 = np.where(valid & (L >= f), (r + 16 - p2) & M32, 0)
                    if (g2 >= kGrowMax).any():
                        self.huge_restarts += 1
                        break
                    incl2 = np.cumsum(g2) & M32
                    before2 = (2 + incl2 - g2) & M32
                    lhs2 = before2 + r + 14
                    stop2 = (L > f) & (~valid | (lhs2 > bs))
                    cur = self._open(g, s, f, S0, True)
                    self._window(cur, j0, wend, S0)
                    cur.wide.append(False)
                    f2 = int(np.argmax(stop2)) if stop2.any() else 64
                    mine = (L > f) & (L < f2)
                    if (mine & (lhs2 == bs)).any():
                        self.edges.add(("inner", "eq"))
                    if f and (mine & (a31[:f + 1].min() < mn)).any():
                        cur.mask_used = True
                    if f2 == 64:
                        carry, pmin, opened = 2 + int(incl2[63]), int(mn[63]), True
                        cur.carried += ("inner",)
                        break
                    if valid[f2] and lhs2[f2] == bs + 1:
                        self.edges.add(("inner", "plus1"))
                    self._close(cur, j0 + f2, f2, before2[f2], "inner", s1, S0)
                    s, f = j0 + f2, f2
                if opened:
                    j0 += 64
                    continue
                break


def oracle_table(blocks, blk_off):
    """(first entry, encoded size) per block of an oracle-encoded stream."""
    off = np.asarray(blk_off, np.int64)
    cnt = pc.block_entry_counts(blocks, off)
    return np.concatenate([[0], np.cumsum(cnt)])[:-1], np.diff(off)


def check_table(W: Walk, blocks, blk_off):
    """The restatement's block table == the oracle's."""
    first, size = W.table()
    ofirst, osize = oracle_table(blocks, blk_off)
    assert len(first) == len(ofirst), f"restatement finds {len(first)} blocks, the oracle {len(ofirst)}"
    bad = np.flatnonzero((first != ofirst) | (size != osize))
    assert bad.size == 0, (f"block {bad[0]}: restatement (first {first[bad[0]]}, size {size[bad[0]]}), "
                           f"oracle (first {ofirst[bad[0]]}, size {osize[bad[0]]})")


def walk_line(name, W: Walk):
    B = W.blocks
    return (f"{name}: {len(B)} blocks; start lanes {len({b.lane0 for b in B})}, end lanes {len({b.f for b in B})}; "
            f"max windows {max((b.windows for b in B), default=0)}; inner-opened {sum(b.inner_opened for b in B)}; "
            f"carried outer/inner {sum('outer' in b.carried for b in B)}/{sum('inner' in b.carried for b in B)}; "
            f"direct {sum(b.direct for b in B)}; straddling windows {len(W.straddles)}; "
            f"wide windows {sum(sum(b.wide) for b in B)} (scan64 {W.scan64}); huge restarts {W.huge_restarts}; "
            f"edges {sorted(W.edges)}")


# ------------------------------------------------------------------------------- pair / tail probes
FIRST_DIFF_Z = tuple(range(20)) + (31, 32, 33)
BYTE_PAIRS = ((0x7F, 0x80), (0x00, 0x01), (0xFE, 0xFF))
PREFIX_M = tuple(range(1, 21))


def _common(z, salt):
    return bytes((37 * i + salt) % 251 + 1 for i in range(z))


def first_diff_probe(z, lo, hi, unsorted, tail=4, salt=0):
    """[F, A, B] with A and B first differing at byte z, by (lo, hi) when sorted and (hi, lo) when
    not; the bytes after the difference are ordered the other way (a whole-dword compare decides
    wrongly).  F = the smaller key's first z + 1 bytes: F <= A always, and in the unsorted probe
    LCP(F, B) = z + 1 > min(LCP(F, A), LCP(A, B)) = z, so a missed detection changes B's prefix."""
    c = _common(z, salt)
    small, large = c + bytes([lo]) + b"\xff" * tail, c + bytes([hi]) + b"\x00" * tail
    a, b = (large, small) if unsorted else (small, large)
    return [small[:z + 1], a, b]


def pair_probes(seed=401):
    """One probe per segment, one block each (block_size 4096): first differences, prefix pairs and
    shortcut-defeating triples.  The unsorted prefix probe (B a prefix of A) takes a fourth entry:
    with three, LCP(F, B) = min(LCP(F, A), |B|) whatever F is, and no byte could change."""
    rng = np.random.default_rng(seed)
    probes = []
    for z in FIRST_DIFF_Z:
        for lo, hi in BYTE_PAIRS:
            for uns in (False, True):
                probes.append(first_diff_probe(z, lo, hi, uns, salt=z))
    for m in PREFIX_M:
        b = _common(m, 100 + m)
        probes.append([b[:1], b, b + b"\x00\x01"])                    # A a prefix of B
        probes.append([b[:1], b, b])                                   # A == B
        # B a prefix of A: F = B + 00 <= A = B + 01, then B, then C = F + 07 with LCP(F, C) = m + 1
        probes.append([b + b"\x00", b + b"\x01", b, b + b"\x00\x07"])
    for lf in (1, 5, 16, 17, 30):
        for k in sorted({0, 3, lf - 1}):
            if k >= lf:
                continue
            f = _common(lf, 200 + lf)
            a = f[:k] + bytes([f[k] + 1]) + b"\x00\x00"
            probes.append([f, a, f + b"\x01\x02\x03"])                 # B = F + suffix < A
    ents, seg = [], [0]
    for pr in probes:
        for k in pr:
            ents.append((k, int(rng.integers(1, 1 << 40)), bytes(rng.integers(0, 256, int(rng.integers(0, 4)), dtype=np.uint8))))
        seg.append(len(ents))
    # a last long key keeps every probe's pairs off the tail route
    ents.append((b"\xff" * 40, 1, b""))
    seg.append(len(ents))
    return O.KV.from_entries(ents), np.asarray(seg, np.uint32), 4096


def tail_probes(seed=402):
    """<= 24 streams (three long keys, then the probe as a segment of its own) whose last two or three keys are 1 to 15 bytes long, so that the
    last pairs start within 16 bytes of the arena's end (the key_diff route): first differences at
    z & 3 = 0..3 sorted and unsorted, and the three prefix kinds."""
    rng = np.random.default_rng(seed)
    lead = [b"\x00" * 24, b"\x00" * 24 + b"\x05", b"\x00\x01" * 9]  # below every probe's first key
    tails = []
    for z in (0, 1, 2, 3, 5, 10):
        for uns in (False, True):
            lo, hi = BYTE_PAIRS[z % 3]
            tails.append(first_diff_probe(z, lo, hi, uns, tail=1 + z % 3, salt=z))
    for m in (1, 4, 6, 13):
        b = _common(m, 50 + m)
        tails.append([b[:1], b, b + b"\x00"])
        tails.append([b[:1], b, b])
        if 2 * m + 2 < 16:  # (B and C both inside the arena's last 16 bytes)
            tails.append([b + b"\x00", b + b"\x01", b, b + b"\x00\x07"])
    assert len(tails) <= 24
    cases = []
    for t in tails:
        assert all(1 <= len(k) <= 15 for k in t[-2:])
        ents = [(k, int(rng.integers(1, 1 << 40)), b"v" * int(rng.integers(0, 3))) for k in lead + t]
        cases.append((O.KV.from_entries(ents), np.asarray([0, len(lead), len(ents)], np.uint32), 4096))
    return cases


# ------------------------------------------------------------------------------- packed streams
class _Pack:
    """Entries added one at a time with BlockBuilder's arithmetic kept beside them (estimated size
    2 + data + 2 per entry; an entry is refused when est + klen + vlen + 14 > block_size and the
    block is not empty), so that a generator can size a value to land on the reject rule's edge."""

    def __init__(self, bs):
        self.bs, self.keys, self.vlen, self.seg = bs, [], [], [0]
        self._new()

    def _new(self):
        self.k0, self.est, self.n = None, 2, 0

    def lhs(self, key, vlen=0):
        return self.est + len(key) + vlen + 14

    def add(self, key, vlen, first=None):
        """first: the entry must (True) / must not (False) start a block."""
        assert vlen >= 0 and len(key) > 0
        starts = self.n == 0 or self.lhs(key, vlen) > self.bs
        assert first is None or first == starts, (len(self.keys), first, self.lhs(key, vlen))
        if starts:
            self._new()
            self.k0 = key
        self.est += len(key) + vlen + 16 - (0 if starts else lcp(self.k0, key))
        self.n += 1
        self.keys.append(key)
        self.vlen.append(vlen)

    def end_segment(self):
        self.seg.append(len(self.keys))
        self._new()

    def build(self, seed):
        rng = np.random.default_rng(seed)
        klen = np.array([len(k) for k in self.keys], np.uint64)
        ko, vo = synth._offsets(klen), synth._offsets(np.asarray(self.vlen, np.uint64))
        keys = np.frombuffer(b"".join(self.keys), np.uint8).copy()
        kv = O.KV(keys, ko, synth._random_bytes(rng, int(vo[-1])), vo, synth._ts(rng, len(klen)))
        return kv, np.asarray(self.seg, np.uint32), self.bs


KLEN = 12


def _key(g, b, i, pattern, kink=-1):
    """[segment u16][block u16][8-byte body].  flat: 0000 + i.  dip: entry 0 all zero, the others
    01000000 + i, so that the block's smallest adjacent LCP (4) is its second entry's and every later
    adjacent LCP is 7 or more.  kink: entry `kink` is 05000000 + i, above its successor (an
    out-of-order pair) and sharing 4 bytes with it, while the successor shares 7 with the block's
    first key: the min shortcut would give 4."""
    head = bytes([g >> 8, g & 255, b >> 8, b & 255])
    lead = 5 if i == kink else (1 if pattern == "dip" and i else 0)
    return head + bytes([lead, 0, 0, 0]) + i.to_bytes(4, "big")


def _script(P: _Pack, g, length, cycle):
    """Segment g: blocks of cycle's (n, mode, pattern[, kink]) in turn until `length` entries.
    Modes size the block's last value: 'exact' fills to the reject rule's left-hand side == block_size,
    'plus1' leaves the next block's first entry at block_size + 1, 'loose' at block_size - 5;
    'single' is a one-entry block whose estimated size is block_size."""
    bs, left, b = P.bs, length, 0
    while left > 0:
        spec = cycle[b % len(cycle)]
        n, mode, pattern = spec[:3]
        kink = spec[3] if len(spec) > 3 else -1
        nxt = cycle[(b + 1) % len(cycle)]
        for i in range(min(n, left)):
            key = _key(g, b, i, pattern, kink)
            v = 0
            if mode == "single":
                v = bs - 18 - KLEN
            elif i == n - 1:
                p = lcp(P.k0, key)
                if mode == "exact":
                    v = bs - P.lhs(key)
                elif mode == "loose":
                    v = bs - 5 - P.lhs(key)
                else:  # est after this entry + the next first entry's klen + 14 == block_size + 1
                    assert nxt[0] >= 2 and nxt[1] != "single"
                    v = bs + 1 - 14 - KLEN - (P.est + KLEN + 16 - p)
            P.add(key, v, first=(i == 0))
        left -= min(n, left)
        b += 1
    P.end_segment()


GEOMETRY_BS = 4096
# cumulative entries: 0, 1, 63, 64, 128, 131, 133, 138, 288, 328, 384, 448
GEOMETRY_A = [(1, "single", "flat"), (62, "exact", "flat"), (1, "single", "flat"), (64, "plus1", "flat"),
              (3, "loose", "flat"), (2, "exact", "flat"), (5, "plus1", "flat"), (150, "exact", "dip"),
              (40, "loose", "flat"), (56, "loose", "flat")] + [(1, "single", "flat")] * 64
# cumulative entries: 0, 150, 187, 277, 282, 283, 353
GEOMETRY_B = [(150, "exact", "dip"), (37, "plus1", "flat"), (90, "loose", "flat"), (5, "exact", "flat"),
              (1, "single", "flat"), (70, "loose", "dip")]


def geometry_lengths():
    return [0, 1, 63, 64, 65, kPipeE - 1, kPipeE + 1, kChunk - 1, kChunk, kChunk + 1, kRing - 1, kRing, kRing + 1,
            kRing + kChunk - 1, kRing + kChunk + 1, 2 * kRing + 1]


def geometry(seed=403):
    """One segment per length of geometry_lengths(), scripts A and B in turn: blocks that start and
    end on lanes 0, 1 and 63, three ends and 64 one-entry blocks in one window, blocks over three
    windows from either carry, and the reject rule's edge on the outer path and in the inner loop."""
    P = _Pack(GEOMETRY_BS)
    for g, n in enumerate(geometry_lengths()):
        _script(P, g, n, GEOMETRY_B if g & 1 else GEOMETRY_A)
    return P.build(seed)


def check_geometry(W: Walk, seg):
    B = W.blocks
    got = np.diff(np.asarray(seg, np.int64)).tolist()
    assert got == geometry_lengths(), "segment lengths"
    for lane in (0, 1, 63):
        assert any(b.lane0 == lane for b in B), f"no block starts at lane {lane}"
        assert any(b.f == lane and b.ended != "segment" for b in B), f"no block ends at lane {lane}"
    assert any(b.f == 0 and b.ended == "segment" for b in B), "no block ends with its segment on a window's edge"
    assert any(b.found == "outer" and b.f == 0 and b.n > 1 for b in B), "no outer stop at lane 0 (f = 0 in the inner loop)"
    ends = {}
    ones = {}
    for b in B:
        w = (b.seg, (b.end - int(seg[b.seg])) // 64)
        ends[w] = ends.get(w, 0) + 1
        if b.n == 1:
            w1 = (b.seg, (b.first - int(seg[b.seg])) // 64)
            ones[w1] = ones.get(w1, 0) + 1
    assert max(ends.values()) >= 3, "no window with three block ends"
    assert max(ones.values()) == 64, "no window of 64 one-entry blocks"
    assert any(b.windows >= 3 and not b.inner_opened and b.carried.count("outer") >= 2 for b in B), \
        "no block over 3 windows carried by the outer path"
    assert any(b.windows >= 3 and b.carried[:1] == ("inner",) for b in B), "no block over 3 windows opened in the inner loop"
    assert any(b.pmin_used and not b.inner_opened for b in B), "no outer-carried block whose min LCP lies in an earlier window"
    assert any(b.pmin_used and b.inner_opened for b in B), "no inner-opened block whose min LCP lies in an earlier window"
    assert any(b.mask_used for b in B), "no inner-opened block with a smaller alcp on a lane <= f"
    for e in (("narrow", "eq"), ("narrow", "plus1"), ("inner", "eq"), ("inner", "plus1")):
        assert e in W.edges, f"reject rule: no {e}"
    assert any(b.ended == "segment" and 0 < b.f < 63 for b in B), "no partial last window"
    for b in B:
        s0 = int(seg[b.seg])
        if (b.first - s0) // kRing != (b.end - 1 - s0) // kRing:
            break
    else:
        raise AssertionError("no block straddles the ring wrap")
    assert any(b.end > int(seg[b.seg]) and (b.end - int(seg[b.seg])) % kRing == 0 and b.ended != "segment" for b in B), \
        "no block ends exactly on the ring wrap"
    assert not any(b.direct for b in B) and not W.straddles


# cumulative entries after a direct block restart at 0: the grid is re-anchored at every block start
DIRECT_CYCLE = [(23, "loose", "flat", 5), (70, "exact", "flat", 66), (37, "loose", "flat"), (51, "plus1", "dip"),
                (9, "loose", "flat")]


def direct_rewrap(seed=404):
    """Two segments longer than 2 kRing; every cycle of five blocks (23, 70, 37, 51, 9 entries) has an
    out-of-order pair in its first block and one in the second window of its second."""
    P = _Pack(4096)
    _script(P, 0, 2 * kRing + 252, DIRECT_CYCLE)
    _script(P, 1, 2 * kRing + 417, DIRECT_CYCLE[1:] + DIRECT_CYCLE[:1])
    return P.build(seed)


def check_direct_rewrap(W: Walk, seg, pairs: Pairs):
    B = W.blocks
    assert (np.diff(np.asarray(seg, np.int64)) > 2 * kRing).all()
    assert W.straddles, "no window straddles the ring wrap"
    assert any(b.direct and b.direct_window >= 1 for b in B), "no block goes direct after a sorted first window"
    assert any(b.direct and b.direct_window == 0 for b in B) and any(not b.direct for b in B)
    assert any(b.direct and b.straddle for b in B), "no direct block's window straddles the ring wrap"
    assert all(64 % b.n for b in B if b.n > 1), "a block length divides 64"
    # a missed out-of-order pair changes bytes: the min shortcut is wrong inside every direct block
    for b in B:
        if b.direct and (~pairs.sorted[b.first:b.end - 1]).any():
            assert shortcut_differs(W.kv, pairs, b.first, b.end), f"block at {b.first}: the shortcut holds"


# ------------------------------------------------------------------------------- fused walkers
def fused_shape(cus, nseg):
    """(nwalk, spw) as encode_locked derives them for the fused launch."""
    walk_wgs = min(cus, (nseg + 1) // 2)
    walk_wgs += walk_wgs & 1
    nwalk = 2 * walk_wgs
    return nwalk, (nseg + nwalk - 1) // nwalk


def fused_multi(cus, seed=405):
    """5 nwalk / 2 + 1 segments (3 per walker) of natural packing at block_size 4096: 16-byte sorted
    keys, 60-140-byte values.  Most segments hold 20-150 entries; every 32nd walker gets (1000, 200, x)
    and every 32nd (kRing + 76, 1000, x), so that its later segments' windows, based at its first
    segment, hold the ring slots kRing - 1 and 0."""
    rng = np.random.default_rng(seed)
    nwalk = 4 * ((cus + 1) // 2)
    nseg = 2 * nwalk + nwalk // 2 + 1
    assert fused_shape(cus, nseg) == (nwalk, 3)
    ln = rng.integers(20, 151, nseg)
    ln[ln % 64 == 0] += 1
    for w in range(nwalk):
        if 3 * w + 2 > nseg:
            break
        if w % 32 == 3:
            ln[3 * w:3 * w + 2] = (1000, 200)
        elif w % 32 == 19:
            ln[3 * w:3 * w + 2] = (kRing + 76, 1000)
    seg = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint32)
    n = int(seg[-1])
    kv = pc._kv(np.full(n, 16), rng.integers(60, 141, n), pc._be(np.arange(n), 4), 4, rng)
    return kv, seg, 4096


def fused_ring_base(seg, spw):
    g = np.arange(len(seg) - 1)
    return np.asarray(seg, np.int64)[(g // spw) * spw]


def check_fused_multi(W: Walk, seg, cus):
    nseg = len(seg) - 1
    nwalk, spw = fused_shape(cus, nseg)
    assert nseg > 2 * nwalk and spw >= 2, (nseg, nwalk, spw)
    ln = np.diff(np.asarray(seg, np.int64))
    assert (ln % 64 != 0).any() and (ln > kRing).any() and len(set(ln.tolist())) > 16
    later = [x for x in W.straddles if x[0] % spw]
    assert later, "no window straddles the ring wrap inside a walker's second or later segment"
    return nwalk, spw


# ------------------------------------------------------------------------------- wide and huge
WIDE_BS = (kNarrowBs - 1, kNarrowBs, 1 << 31, (1 << 32) - 1)


def wide():
    """~3000 U entries in 2 segments at block sizes on both sides of `narrow`."""
    kv = O.KV(*synth.gen_uniform(3000, seed=406))
    seg = np.asarray([0, 1487, kv.n], np.uint32)
    return [(kv, seg, bs) for bs in WIDE_BS]


def check_wide(W: Walk, bs):
    wide_w = [w for b in W.blocks for w in b.wide]
    assert len(W.blocks) == 2 and all(b.windows >= 23 for b in W.blocks)
    assert all(wide_w) if bs >= kNarrowBs else not any(wide_w), f"block_size {bs}: the wrong path"


def _small(P, g, grp, i, v=0, first=None):
    P.add(bytes([g, grp]) + i.to_bytes(4, "big"), v, first)


def huge(seed=407):
    """[(kv, seg, 4096), (kv2, seg2, 2^25 + 4096)].  First case: per r in (kHugeRec - 1, kHugeRec) three
    segments, the entry of that r (a 6-byte key, the rest value)
      * first in its segment, five small entries after it;
      * at lane 10 of the second window: a block carried into that window ends at lane 6 (the reject
        rule at block_size + 1), a block of four follows, and the inner
        loop meets the entry (its key shares no byte with its predecessor's: growth r + 16);
      * at lane 6 of the second window, inside the block carried into it, whose last entry (lane 5)
        fills it to exactly block_size.
    Second case: one segment, the entry of r = kHugeRec is accepted into the block carried into the
    second window (the 64-bit path with a carry), which then runs on over a third window."""
    def seg_first(P, g, r):
        P.add(bytes([g, 9]) + b"\0\0\0\0", r - 6, True)
        for i in range(5):
            _small(P, g, 10, i, 3, first=(i == 0))  # (refused by a block that is already over block_size)
        P.end_segment()

    def seg_middle(P, g, r):
        for i in range(69):
            _small(P, g, 1, i, 20)
        # lane 5 pads so that lane 6's entry (klen 6, vlen 0) is refused at block_size + 1
        key = bytes([g, 1]) + (69).to_bytes(4, "big")
        v = P.bs + 1 - 14 - 6 - (P.est + 6 + 16 - lcp(P.k0, key))
        P.add(key, v, False)
        for i in range(4):
            _small(P, g, 2, i, 0, first=(i == 0))
        P.add(bytes([g + 1, 0]) + b"\0\0\0\0", r - 6, True)
        for i in range(3):
            _small(P, g + 1, 1, i, 3, first=(i == 0))
        P.end_segment()

    def seg_carried(P, g, r, accept=False):
        for i in range(69):
            _small(P, g, 1, i, 20)
        key = bytes([g, 1]) + (69).to_bytes(4, "big")
        if accept:  # the entry joins the block (it shares 5 key bytes with the first), 17-byte entries follow
            P.add(key, 20, False)
            _small(P, g, 1, 70, r - 6, first=False)
            for i in range(71, 191):
                _small(P, g, 1, i, 0)
        else:
            P.add(key, P.bs - P.lhs(key), False)  # exactly block_size
            P.add(bytes([g + 1, 0]) + b"\0\0\0\0", r - 6, first=True)
            for i in range(3):
                _small(P, g + 1, 1, i, 30, first=(i == 0))
        P.end_segment()

    P = _Pack(4096)
    g = 0
    for r in (kHugeRec - 1, kHugeRec):
        seg_first(P, g, r)
        seg_middle(P, g + 2, r)
        seg_carried(P, g + 4, r)
        g += 6
    Q = _Pack(kHugeRec + 16 + 4096)
    seg_carried(Q, 0, kHugeRec, accept=True)
    return [P.build(seed), Q.build(seed + 1)]


def check_huge(W: Walk, which):
    B = W.blocks
    if which == 0:
        assert W.huge_restarts >= 1, "the inner loop never meets a growth >= kGrowMax"
        assert W.scan64 >= 3, "no 64-bit scan"
        assert W.narrow_near_huge >= 3, "r = kHugeRec - 1 never on the u32 path"
        assert ("wide", "eq") in W.edges and ("wide", "plus1") in W.edges, f"reject rule on the 64-bit path: {W.edges}"
        assert any(b.windows == 2 and b.wide == [False, True] and b.found == "outer" for b in B), \
            "no carried block that meets the 64-bit path in its second window"
        hr = [b for b in B if W.rec[b.first] >= kHugeRec - 1]
        assert len(hr) == 6 and all(b.n == 1 for b in hr)
        assert {b.inner_opened for b in hr if W.rec[b.first] == kHugeRec - 1} == {False, True}
    else:
        big = [b for b in B if (W.rec[b.first:b.end] >= kHugeRec).any()]
        assert len(big) == 1 and big[0].windows >= 3 and big[0].wide[:3] == [False, True, False], \
            "the huge entry is not accepted into a carried block"
        assert big[0].size > kHugeRec
