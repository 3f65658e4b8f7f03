"""Inputs on the edge between walk_segment's anchored pass and its carried-window loop -- TEST
INFRASTRUCTURE, beside tests/walk_cases.py (whose generators and constants it uses).

walk_segment (lsm_amd/csrc/lsmblk_gpu.hip) opens every block with the window [s, s + 64) anchored at
the block's first entry s: lane 0 is entry s, the estimated size starts at 2, and one min-scan, one
sum-scan and one ballot find the block's end when it has at most 64 entries.  A block still open at
lane 63, a window with an out-of-order pair, and the 64-bit arithmetic go to the carried-window loop
(walk_cases.Walk restates that loop on its fixed 64-entry grid).

  AnchoredWalk   lane-level restatement of the walk with the anchored pass in front.  Its block table
                 must equal the oracle's; then what it says about routes and lanes can be trusted.
  edges()        one stream, one segment per edge (see SEGMENTS).

The restatement only ASSERTS COVERAGE.  Expected bytes come from the oracle.
"""
from dataclasses import dataclass

import numpy as np

import walk_cases as wc

kRing, kAlcpLcp, kNarrowBs, kHugeRec, kGrowMax = wc.kRing, wc.kAlcpLcp, wc.kNarrowBs, wc.kHugeRec, wc.kGrowMax
UNSORTED, M32 = wc.UNSORTED, wc.M32


@dataclass
class ABlk:
    seg: int
    first: int
    route: str           # 'anchored': ended by the anchored pass; 'open': no stop on its 64 lanes;
                         # 'direct' / 'wide': the anchored pass did not apply; 'inner': found by the
                         # carried loop's inner loop on the lanes after another block's end
    straddle: bool       # its anchored window holds ring slots kRing - 1 and 0
    unsorted_lanes: tuple = ()  # lanes of its anchored window that hold an out-of-order pair's flag
    end: int = 0
    size: int = 0
    f: int = -1          # lane of the stop that ended it
    windows: int = 1     # windows it was read through
    at_segment_end: bool = False

    @property
    def n(self):
        return self.end - self.first


class AnchoredWalk:
    """walk_segment over (rec, alcp) per entry.  ring_base[g]: the entry at ring slot 0 for segment g."""

    def __init__(self, kv, seg, block_size, ring_base=None):
        self.kv, self.bs = kv, int(block_size)
        self.seg = np.asarray(seg, np.int64)
        self.alcp = wc.classify_pairs(kv, seg).alcp
        self.rec = np.diff(kv.key_off.astype(np.int64)) + np.diff(kv.val_off.astype(np.int64))
        self.blocks, self.edges = [], set()
        base = self.seg[:-1] if ring_base is None else np.asarray(ring_base, np.int64)
        for g in range(len(self.seg) - 1):
            self._segment(g, int(self.seg[g]), int(self.seg[g + 1]), int(base[g]))

    def table(self):
        return (np.array([b.first for b in self.blocks], np.int64), np.array([b.size for b in self.blocks], np.int64))

    def _close(self, b, end, f, size, s1):
        b.end, b.f, b.size, b.at_segment_end = end, f, int(size) & M32, end == s1

    def _segment(self, g, s0, s1, S0):
        rec, alcp, bs = self.rec, self.alcp, self.bs
        narrow = bs < kNarrowBs
        L = np.arange(64)
        s = s0
        while s < s1:
            carry, pmin, direct = 2, kAlcpLcp, False
            j0 = s
            # ---- the anchored pass
            e = s + L
            valid = e < s1
            ec = np.minimum(e, s1 - 1)
            r = np.where(valid, rec[ec], 0)
            al = np.where(valid & (L > 0), alcp[ec], kAlcpLcp)
            straddle = ((s - S0) & (kRing - 1)) + (min(s1, s + 64) - s) > kRing
            uns = tuple(np.flatnonzero(al & UNSORTED).tolist())
            cur = ABlk(g, s, "", straddle, uns)
            self.blocks.append(cur)
            if narrow and not uns and not (valid & (r >= kHugeRec)).any():
                mn = np.minimum.accumulate(al)
                g32 = np.where(valid, (r + 16 - np.where(L > 0, mn, 0)) & M32, 0)
                i32 = np.cumsum(g32) & M32
                b32 = (2 + i32 - g32) & M32
                lhs = (b32 + r + 14) & M32
                stop = (L > 0) & (~valid | (lhs > (bs & M32)))
                f = int(np.argmax(stop)) if stop.any() else 64
                if ((L > 0) & (L < f) & (lhs == bs)).any():
                    self.edges.add(("anchored", "eq"))
                if f < 64:
                    if valid[f] and lhs[f] == bs + 1:
                        self.edges.add(("anchored", "plus1"))
                    cur.route = "anchored"
                    self._close(cur, s + f, f, b32[f], s1)
                    s += f
                    continue
                cur.route = "open"
                carry, pmin, j0 = 2 + int(i32[63]), int(mn[63]), s + 64
            else:
                cur.route = "direct" if uns else "wide"
                cur.windows = 0
            # ---- the carried-window loop (as walk_cases.Walk._segment)
            while True:
                e = j0 + L
                valid = e < s1
                ec = np.minimum(e, max(s1 - 1, 0))
                r = np.where(valid, rec[ec], 0)
                al = np.where(valid & (e != s), alcp[ec], kAlcpLcp)
                cur.windows += 1
                if not direct and (al & UNSORTED).any():
                    direct = True
                a31 = al & kAlcpLcp
                if not direct:
                    p = np.minimum(pmin, np.minimum.accumulate(a31))
                    pmin = int(p[63])
                else:
                    p = np.zeros(64, np.int64)
                    for l in np.flatnonzero(valid & (e != s)):
                        p[l] = wc.lcp(wc.key_of(self.kv, s), wc.key_of(self.kv, int(e[l])))
                p = np.where(e == s, 0, p)
                if narrow and not (valid & (r >= kHugeRec)).any():
                    g32 = np.where(valid, (r + 16 - p) & M32, 0)
                    i32 = np.cumsum(g32) & M32
                    before = ((carry & M32) + i32 - g32) & M32
                    stop = ~valid | ((e != s) & (((before + r + 14) & M32) > (bs & M32)))
                    incl_all = int(i32[63])
                else:
                    gr = np.where(valid, r + 16 - p, 0)
                    incl = np.cumsum(gr)
                    if (gr < kGrowMax).all():
                        incl &= M32
                    before = carry + incl - gr
                    stop = ~valid | ((e != s) & (before + r + 14 > bs))
                    incl_all = int(incl[63])
                if not stop.any():
                    carry += incl_all
                    j0 += 64
                    continue
                f = int(np.argmax(stop))
                self._close(cur, j0 + f, f, before[f], s1)
                s = j0 + f
                opened = False
                while not direct and s < s1:
                    mn = np.minimum.accumulate(np.where(L <= f, kAlcpLcp, a31))
                    g2 = np.where(valid & (L >= f), (r + 16 - np.where(L <= f, 0, mn)) & M32, 0)
                    if (g2 >= kGrowMax).any():
                        break
                    incl2 = np.cumsum(g2) & M32
                    before2 = (2 + incl2 - g2) & M32
                    stop2 = (L > f) & (~valid | (before2 + r + 14 > bs))
                    cur = ABlk(g, s, "inner", False)
                    self.blocks.append(cur)
                    if not stop2.any():
                        carry, pmin, opened = 2 + int(incl2[63]), int(mn[63]), True
                        break
                    f2 = int(np.argmax(stop2))
                    self._close(cur, j0 + f2, f2, before2[f2], s1)
                    s, f = j0 + f2, f2
                if opened:
                    j0 += 64
                    continue
                break


def check_table(W: AnchoredWalk, blocks, blk_off):
    """The restatement's block table == the oracle's."""
    first, size = W.table()
    ofirst, osize = wc.oracle_table(blocks, blk_off)
    assert len(first) == len(ofirst), f"restatement finds {len(first)} blocks, the oracle {len(ofirst)}"
    bad = np.flatnonzero((first != ofirst) | (size != osize))
    assert bad.size == 0, (f"block {bad[0]}: restatement (first {first[bad[0]]}, size {size[bad[0]]}), "
                           f"oracle (first {ofirst[bad[0]]}, size {osize[bad[0]]})")


def walk_line(name, W: AnchoredWalk):
    B = W.blocks
    by = {r: sum(b.route == r for b in B) for r in ("anchored", "open", "direct", "wide", "inner")}
    return (f"{name}: {len(B)} blocks by route {by}; anchored end lanes {len({b.f for b in B if b.route == 'anchored'})}; "
            f"straddling anchored windows {sum(b.straddle for b in B)}; edges {sorted(W.edges)}")


# ------------------------------------------------------------------------------- the edge stream
BS = 4096
# blocks of 63, 64 and 65 twelve-byte keys and empty values, the last value filling the block to the
# reject rule's edge: the first rejected entry is the 64th, 65th or 66th, refused at block_size + 1
# ('plus1') or after a block filled to exactly block_size ('exact')
EDGE = [(63, "exact", "flat"), (64, "plus1", "flat"), (65, "exact", "flat"), (64, "exact", "flat"),
        (63, "plus1", "flat"), (65, "plus1", "flat"), (3, "loose", "flat")]
# a block over three windows, then short ones on the lanes after its end
LONG = [(150, "exact", "dip"), (3, "loose", "flat"), (2, "exact", "flat"), (5, "plus1", "flat"), (40, "loose", "flat"),
        (130, "plus1", "flat"), (7, "loose", "flat")]
# an out-of-order pair whose flag sits on lane 1 (entry 0 above entry 1) and on lane 63 of the anchored window
KINK = [(23, "loose", "flat", 0), (70, "exact", "flat", 62), (37, "loose", "flat"), (9, "loose", "flat")]
# block lengths that share no factor with the ring: anchored windows start on every kind of slot
RING = [(37, "loose", "flat"), (51, "plus1", "dip"), (9, "loose", "flat"), (29, "exact", "flat")]
SEGMENTS = ([(1, EDGE), (65, [(65, "loose", "flat")]), (64, [(64, "loose", "flat")]), (127, EDGE)] +
            # (one edge block first in its segment each: once a block has gone to the carried loop, the loop
            # keeps the rest of the segment)
            [(n + 5, [(n, mode, "flat"), (5, "loose", "flat")]) for n in (63, 64, 65) for mode in ("exact", "plus1")] +
            [(2 * sum(c[0] for c in EDGE), EDGE), (700, LONG), (400, KINK), (kRing + 300, RING), (65, RING)])


def edges(seed=431):
    P = wc._Pack(BS)
    for g, (n, cycle) in enumerate(SEGMENTS):
        wc._script(P, g, n, cycle)
    return P.build(seed)


def check_edges(W: AnchoredWalk, seg):
    B = W.blocks
    ln = np.diff(np.asarray(seg, np.int64)).tolist()
    assert ln == [n for n, _ in SEGMENTS] and 1 in ln and 65 in ln
    for e in (("anchored", "eq"), ("anchored", "plus1")):
        assert e in W.edges, f"reject rule in the anchored pass: no {e}"
    # 63 entries: ended by the anchored pass on lane 63; 64 and 65: open, ended by the carried loop on lanes 0 and 1
    # (each at least twice: the last entry filling the block exactly, and the next one refused by one byte)
    assert sum(b.n == 63 and b.route == "anchored" and b.f == 63 for b in B) >= 2
    assert sum(b.n == 64 and b.route == "open" and b.f == 0 and b.windows == 2 and not b.at_segment_end for b in B) >= 2
    assert sum(b.n == 65 and b.route == "open" and b.f == 1 and b.windows == 2 and not b.at_segment_end for b in B) >= 2
    assert not any(b.route == "anchored" and b.n > 63 for b in B) and not any(b.route == "open" and b.n < 64 for b in B)
    # a 64-entry block that ends exactly at s1: as a whole segment, and after another block
    at_end = [b for b in B if b.n == 64 and b.route == "open" and b.at_segment_end]
    assert any(b.first == int(seg[b.seg]) for b in at_end) and any(b.first > int(seg[b.seg]) for b in at_end)
    # the one-entry segment: lane 1 is past s1
    assert any(b.n == 1 and b.route == "anchored" and b.f == 1 and b.at_segment_end for b in B)
    assert any(b.straddle and b.route == "anchored" for b in B), "no anchored window wraps the ring"
    # a block longer than 64 entries, then short ones found on the same window's later lanes
    for i, b in enumerate(B[:-2]):
        if b.n > 128 and b.route == "open" and B[i + 1].route == "inner" and B[i + 2].route == "inner" and B[i + 1].n < 8:
            break
    else:
        raise AssertionError("no long block followed by short ones")
    # (the carried loop keeps the rest of the segment: every later block of it starts on a lane of a
    # grid window; the next segment is anchored again)
    rest = [c for c in B[i + 1:] if c.seg == b.seg]
    assert len(rest) > 8 and all(c.route == "inner" for c in rest) and any(c.n > 64 for c in rest)
    assert B[i + 1 + len(rest)].route in ("anchored", "direct")
    assert any(b.route == "direct" and b.unsorted_lanes == (1,) for b in B), "no out-of-order pair at lane 1"
    assert any(b.route == "direct" and b.unsorted_lanes == (63,) for b in B), "no out-of-order pair at lane 63"
