"""Inputs that put the entries of a block on chosen routes of the decode -- TEST INFRASTRUCTURE.

The method of path_cases.py, crc_cases.py and walk_cases.py, one level down: path_cases.py chooses
the block's path, this file the routes inside a block (dec_entry_runs, dec_fast_outputs,
dec_big_entry, dec_big_outputs, copy_run, copy_long_runs / copy_issue, st_short,
dec_simple_outputs in lsmblk_gpu.hip, flush_chunks / store_chunk in lsmblk_dev.hpp).  Shared by
test_decode_cases.py (CPU) and test_gpu_decode_routes.py (GPU):

  constants    kDecImg, kDecMaxE, kDecOut, kLB, kBigB, kDecBigB (LSMBLK_XDBB), kCoop, kCopyScratch
               and kTile, read out of the sources.
  model        model_block(): a plain Python restatement of which route every entry of a block
               takes and with which parameters, as a set of events (tuples).  Inputs: the block's
               bytes, the low four bits of its address (lead) and its output bases K0, V0.  The
               model is never the expected output: it only says which route an input reaches, and
               the check_* functions are set inclusions over its events.
  writer       block(): a block assembled by hand from entries (p, suffix, ts, value) at chosen
               data positions, an offset table in any order and gap bytes; expected entries come
               from pyref.block_entries and the C oracle.
  generators   keys_fast, values_fast, impossible, amplified, large, simple.  A block under test
               is preceded by a one-entry filler block that sets K0 & 15 and V0 & 15.  Key tails
               and values are random bytes in [1, 0xE0); gaps and padding are GAP, so a read from
               the wrong place shows.

A check_* function takes the constants it checks against, so a batch built for other constants, or
a cut-down generator, fails it.
"""
import os
import re
import struct
from dataclasses import dataclass

import numpy as np

import path_cases as pc
from oracle import pyref

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsm_amd", "csrc")
GPU_SRC = os.path.join(_CSRC, "lsmblk_gpu.hip")
LITERALS = ("kDecImg", "kDecMaxE", "kDecOut", "kLB", "kBigB", "kCoop", "kTile")
GAP = 0xEE        # gaps, padding
FILL = 0xA5       # the GPU test's output prefill
LEADS = (0, 1, 8, 15)


@dataclass(frozen=True)
class Consts:
    kDecImg: int
    kDecMaxE: int
    kDecOut: int
    kLB: int
    kBigB: int
    kCoop: int
    kTile: int
    kDecBigB: int
    kCopyScratch: int


def kernel_constants(path=GPU_SRC):
    """The decode's constants.  The literal ones through path_cases.read_constants; kDecBigB is
    `constexpr uint32_t kDecBigB = LSMBLK_XDBB;` with the macro's default, kCopyScratch a sum of
    products of literals."""
    out = pc.read_constants(path, LITERALS)
    with open(path) as f:
        text = f.read()
    if not re.search(r"^constexpr\s+uint32_t\s+kDecBigB\s*=\s*LSMBLK_XDBB\s*;", text, re.M):
        raise RuntimeError(f"kDecBigB: no `constexpr uint32_t kDecBigB = LSMBLK_XDBB;` in {path}")
    m = re.search(r"^#\s*define\s+LSMBLK_XDBB\s+(\d+)\s*$", text, re.M)
    if not m:
        raise RuntimeError(f"LSMBLK_XDBB: no default in {path}")
    out["kDecBigB"] = int(m.group(1))
    m = re.search(r"^constexpr\s+uint32_t\s+kCopyScratch\s*=\s*([0-9 +*]+);", text, re.M)
    if not m:
        raise RuntimeError(f"kCopyScratch: no `constexpr uint32_t kCopyScratch = <sum of products>;` in {path}")
    out["kCopyScratch"] = sum(int(np.prod([int(f) for f in term.split("*")])) for term in m.group(1).split("+"))
    return Consts(**out)


C = kernel_constants()


# ------------------------------------------------------------------------------- the writer
def rb(rng, n):
    """n random bytes in [1, 0xE0): never 0, never GAP."""
    return rng.integers(1, 0xE0, int(n), dtype=np.uint8).tobytes()


def block(entries, order=None, gaps=None, tailgap=0):
    """A block from physical entries (p, suffix, ts, value) laid out in the given order, gaps[i]
    GAP bytes before entry i (entry 0 sits at data position 0: gaps[0] must be 0), tailgap GAP
    bytes between the last entry and the offset table, and an offset table that names the physical
    entries in `order` (any order, repeats allowed; default 0 .. len - 1)."""
    gaps = gaps or [0] * len(entries)
    assert gaps[0] == 0 and len(gaps) == len(entries)
    data, pos = bytearray(), []
    for (p, sfx, ts, val), g in zip(entries, gaps):
        data += bytes([GAP]) * g
        pos.append(len(data))
        data += struct.pack(">HH", p, len(sfx)) + sfx + struct.pack(">QH", ts, len(val)) + val
    data += bytes([GAP]) * tailgap
    assert max(pos) < 65536
    order = list(range(len(entries))) if order is None else list(order)
    assert 0 < len(order) < 65536
    return bytes(data) + b"".join(struct.pack(">H", pos[i]) for i in order) + struct.pack(">H", len(order))


def parse(buf):
    """-> (n, data_end, fks, [(epos, p, s, vl)] in offset-table order)."""
    L = len(buf)
    n = struct.unpack_from(">H", buf, L - 2)[0]
    de = L - 2 - 2 * n
    fks = struct.unpack_from(">H", buf, 2)[0]
    ents = []
    for k in range(n):
        off = struct.unpack_from(">H", buf, de + 2 * k)[0]
        p, s = struct.unpack_from(">HH", buf, off)
        vl = struct.unpack_from(">H", buf, off + 12 + s)[0]
        assert off + 14 + s + vl <= de and p <= fks and p + s > 0
        ents.append((off, p, s, vl))
    return n, de, fks, ents


class Batch:
    """Blocks back to back.  K, V: the decoded key / value bytes so far (the next block's K0, V0)."""

    def __init__(self, name, seed):
        self.name, self.rng = name, np.random.default_rng(seed)
        self.bufs, self.tags, self.K0, self.V0 = [], [], [], []
        self.K = self.V = self.size = 0

    def ts(self):
        return int(self.rng.integers(0, 1 << 63))

    def add(self, buf, tag):
        _, _, _, ents = parse(buf)
        self.bufs.append(buf)
        self.tags.append(tag)
        self.K0.append(self.K)
        self.V0.append(self.V)
        self.K += sum(p + s for _, p, s, _ in ents)
        self.V += sum(vl for _, _, _, vl in ents)
        self.size += len(buf)

    def case(self, buf, tag, kb=None, vb=None, at=None):
        """`buf` after a one-entry filler block that makes K0 & 15 == kb and V0 & 15 == vb (random
        when None); at: also the block's stream offset & 15 (by gap bytes in the filler)."""
        kb = int(self.rng.integers(16)) if kb is None else kb
        vb = int(self.rng.integers(16)) if vb is None else vb
        fk, fv = (kb - self.K - 1) % 16 + 1, (vb - self.V) % 16
        tg = 0 if at is None else (at - (self.size + 18 + fk + fv)) % 16
        self.add(block([(0, rb(self.rng, fk), self.ts(), rb(self.rng, fv))], tailgap=tg), "filler")
        assert self.K % 16 == kb and self.V % 16 == vb and (at is None or self.size % 16 == at)
        self.add(buf, tag)

    @property
    def blocks(self):
        return np.frombuffer(b"".join(self.bufs), np.uint8)

    @property
    def blk_off(self):
        return np.concatenate([[0], np.cumsum([len(b) for b in self.bufs])]).astype(np.uint64)

    def entries(self):
        """pyref.block_entries of every block, concatenated."""
        return [e for b in self.bufs for e in pyref.block_entries(b)]


# ------------------------------------------------------------------------------- the model
def _nf_class(nf):
    return 0 if nf <= 0 else "whole" if nf >= 4 else nf


def _short_class(ln):
    """put_short / st_short by length: bytes, 4+4, or 8+8 with x = len - 8 below or at least 4."""
    return "1-3" if ln < 4 else "4-7" if ln < 8 else "8-15,x<4" if ln - 8 < 4 else "8-15,x>=4"


def _flush(ev, run, lo, ln, c):
    if ln == 0:
        ev.add(("flush-empty", run))
        return
    end = lo + ln
    nc = (end + 15) >> 4
    head, tail = lo != 0 or end < 16, (end & 15) != 0
    nw = max((nc - 1 if tail else nc) - (1 if head else 0), 0)
    ev.add(("flush", lo, end & 15))
    ev.add(("flush-edges", run, head, tail, end < 16))
    ev.add(("flush-whole", "0" if nw == 0 else "<" if nw < 64 * c.kLB else "=" if nw == 64 * c.kLB else ">"))


def _fast(ev, ents, lead, kb, vb, K, V, c):
    n = len(ents)
    vrun = (kb + K + 15) & ~15
    lds = vrun + ((vb + V + 15) & ~15) <= c.kDecOut
    sink = "lds" if lds else "glb"
    ev.add(("sink", sink))
    fk = lead + 4
    kout = np.concatenate([[0], np.cumsum([p + s for _, p, s, _ in ents])])
    vout = np.concatenate([[0], np.cumsum([vl for _, _, _, vl in ents])])
    outvb = vrun + vb if lds else vb
    for it in range(2):
        if 64 * it >= n:
            break
        lanes = range(64 * it, min(n, 64 * it + 64))
        sb = {k: lead + ents[k][0] + 4 for k in lanes}
        kuni = not any(ents[k][1] + ents[k][2] < 16 or sb[k] < ents[k][1] for k in lanes)
        nkmax = max((ents[k][1] + ents[k][2] + 15) >> 4 for k in lanes)
        nvmax = max([(ents[k][3] + 15) >> 4 for k in lanes if ents[k][3] >= 16] or [0])
        ev.add(("kuni", kuni, sink))
        # valn and the terms that turn it off
        vS0, vD0 = sb[64 * it] + ents[64 * it][2] + 10, outvb + int(vout[64 * it])
        terms = set()
        if not lds:
            terms.add("sink")
        if n > 64:
            terms.add("n")
        if any(ents[k][3] < 16 for k in lanes):
            terms.add("short")
        if vS0 < (vD0 & 15):
            terms.add("lane0")
        valn = not terms
        ev.add(("valn", valn))
        ev.update(("valn-term", t) for t in terms)
        if len(terms) == 1:
            ev.add(("valn-off-alone", next(iter(terms))))
        if it == 1:
            ev.add(("second-half", sink, len(lanes)))
        vm_max = 0
        for k in lanes:
            epos, p, s, vl = ents[k]
            kl, l = p + s, k - 64 * it
            kD = kb + int(kout[k])
            ev.add(("key", kl, p))
            ev.add(("key-align", kuni, kD & 15))
            if s == 0:
                ev.add(("key-s0", p > 0))

            def merged(o):
                for d in range(4):
                    ev.add(("nf", d, _nf_class(p - (o + 4 * d))))
                if p - o > 0:
                    ev.add(("p-in-piece", min(p - o, 16)))
            if kuni:
                ev.add(("kpieces", (kl + 15) >> 4, nkmax))
                for t in range(nkmax):
                    o = min(16 * t, kl - 16)
                    merged(o)
                    ev.add(("kclamp", 16 * t > kl - 16, (kl - 16) & 15))
            else:
                for t in range(0, kl, 16):
                    o = min(t, kl - 16) if kl >= 16 else 0
                    if sb[k] + o >= p:
                        merged(o)
                    else:
                        ev.add(("key-bytes", "index0" if k == 0 else "index>0", sink))
                if kl < 16:
                    ev.add(("kshort", sink, kl))
                    ev.add(("kshort-class", sink, _short_class(kl)))
            vS, vD = sb[k] + s + 10, outvb + int(vout[k])
            if valn:
                cs = (vD >> 4) if l == 0 else ((vD + 15) >> 4)
                ce = (vD + vl - 1) >> 4
                vm = ce - cs + 1
                vm_max = max(vm_max, vm)
                a0 = vS + 16 * cs - vD
                assert a0 >= 0 and vm >= 1
                ev.add(("vpair", vD & 15, vl & 15))
                ev.add(("a0&7", a0 & 7))
                ev.add(("vm", vm))
                if l == 0:
                    ev.add(("lane0-chunk", vD & 15))
                for ch in range(cs, ce + 1):
                    cut = vD + vl - 16 * ch
                    if cut < 16:
                        ev.add(("cut", cut, "next" if k + 1 < n else "last"))
                        if k + 1 < n:
                            a1 = sb[k + 1] + ents[k + 1][2] + 10 + 16 * ch - (vD + vl)
                            assert a1 >= 0
                            ev.add(("a1&7", a1 & 7))
                            if a1 < 16:
                                ev.add(("a1", a1))
                    elif ch == ce:
                        ev.add(("cut", 16, "next" if k + 1 < n else "last"))
            else:
                ev.add(("vl", vl, vD & 15, sink))
                if vl >= 16:
                    np_ = (vl + 15) >> 4
                    ev.add(("vpieces", np_, nvmax, -(-nvmax // c.kLB)))
                    for i in range(-(-nvmax // c.kLB) * c.kLB):
                        ev.add(("vclamp", 16 * i > vl - 16))
                elif vl:
                    ev.add(("vshort", sink, vl))
                    ev.add(("vshort-class", sink, _short_class(vl)))
                else:
                    ev.add(("vempty", sink))
        if valn:
            ev.add(("valn-n", n))
            ev.add(("vmmax", vm_max))
    if lds:
        _flush(ev, "keys", kb, K, c)
        _flush(ev, "vals", vb, V, c)


def _big(ev, ents, lead, ln, c):
    """One table chunk (at most kDecMaxE entries) of a large block: dec_big_outputs."""
    fk, lim = lead + 4, lead + ln
    for c0 in range(0, len(ents), 64):
        lanes = ents[c0:c0 + 64]
        nps = []
        for epos, p, s, vl in lanes:
            sb, kl = lead + epos + 4, p + s
            ev.add(("bkey", kl, p))
            for t in range(0, kl, 16):
                o = min(t, kl - 16) if kl >= 16 else 0
                fails = [i for i, ok in enumerate((sb + o >= p, sb + o - p + 16 <= lim, fk + o + 16 <= lim)) if not ok]
                if not fails:
                    ev.add(("bkey-route", "merged"))
                    for d in range(4):
                        ev.add(("bnf", d, _nf_class(p - (o + 4 * d))))
                else:
                    ev.add(("bkey-route", "bytes", fails[0]))
                    ev.add(("bkey-bytes-around-p", o <= p < o + 16))
            if kl < 16:
                ev.add(("bkshort", kl))
            vsrc = lead + epos + 14 + s
            if vl >= c.kCoop:
                nps.append((vl + 15) >> 4)
                ev.add(("long-value", vl))
            else:
                nps.append(0)
                if vl >= 16:
                    ev.add(("copy_run-long", -(-((vl + 15) >> 4) // c.kBigB)))
                elif vl:
                    ev.add(("copy_run-short", "load16" if vsrc + 16 <= lim else "bytes", vl))
                    ev.add(("bvshort-class", _short_class(vl)))
                else:
                    ev.add(("copy_run-empty",))
        total = sum(nps)
        ev.add(("clr-total", total))
        if total == 0:
            continue
        B = c.kDecBigB
        ev.add(("clr-rows", -(-total // 64)))
        ev.add(("clr-rounds", -(-total // (64 * B))) if total <= 128 * B else ("clr-rounds-many",))
        first = np.concatenate([[0], np.cumsum(nps)])
        starts = {int(first[i]) for i, q in enumerate(nps) if q}
        for r in range(1, -(-total // 64)):
            ev.add(("clr-carry", 64 * r not in starts))
        for i, q in enumerate(nps):
            if q:
                ev.add(("clr-span", (int(first[i]) + q - 1) // 64 - int(first[i]) // 64))
                ev.add(("clr-round-span", (int(first[i]) + q - 1) // (64 * B) - int(first[i]) // (64 * B)))
        own = [i for i, q in enumerate(nps) if q]
        holes = sum(1 for i, q in enumerate(nps) if not q and own[0] < i < own[-1])
        ev.add(("clr-holes", "none" if holes == 0 else "some" if holes < 16 else "many"))


def model_block(buf, lead, K0, V0, c=C):
    """The routes block `buf` takes at address & 15 == lead with output bases K0, V0 -> a set of
    events.  ("path", p) is the block path in path_cases.DEC_PATHS' words."""
    ev = set()
    n, de, fks, ents = parse(buf)
    ln = len(buf)
    K, V = sum(p + s for _, p, s, _ in ents), sum(vl for _, _, _, vl in ents)
    kb, vb = K0 & 15, V0 & 15
    fits = lead + ln + 15 <= c.kDecImg
    if fits and n <= c.kDecMaxE:
        _fast(ev, ents, lead, kb, vb, K, V, c)
        ev.add(("path", "fast-lds" if ("sink", "lds") in ev else "fast-global"))
    elif fits:
        ev.add(("path", "staged-simple"))
        ev.add(("simple", "lds", n))
        for _, p, s, vl in ents:
            ev.add(("simple-entry", p > 0, s > 0, vl > 0))
    elif n <= c.kDecMaxE:
        ev.add(("path", "big-tables"))
        _big(ev, ents, lead, ln, c)
    else:
        ev.add(("path", "big-chunked"))
        ev.add(("table-chunks", n, -(-n // c.kDecMaxE), n - (n - 1) // c.kDecMaxE * c.kDecMaxE))
        for c0 in range(0, n, c.kDecMaxE):
            _big(ev, ents[c0:c0 + c.kDecMaxE], lead, ln, c)
            if c0 and ents[c0 - 1][3] >= c.kCoop:
                ev.add(("long-value-before-table-edge", c0))
    return ev


def model_batch(b: Batch, addr=0, c=C, only=None):
    """Union of the events of every block of the batch but the fillers (only: a tag prefix), the
    stream at address `addr` -> (events, [path per block, fillers included])."""
    ev, paths, off = set(), [], 0
    for buf, tag, K0, V0 in zip(b.bufs, b.tags, b.K0, b.V0):
        e = model_block(buf, (addr + off) & 15, K0, V0, c)
        paths.append(next(x[1] for x in e if x[0] == "path"))
        if tag != "filler" and (only is None or tag.startswith(only)):
            ev |= e
        off += len(buf)
    return ev, paths


def model_leads(b: Batch, leads=LEADS, base=0, c=C, only=None):
    """Union of model_batch over the stream placed at base + lead for every lead."""
    ev = set()
    for ld in leads:
        ev |= model_batch(b, base + ld, c, only)[0]
    return ev


def missing(ev, want):
    return sorted(set(want) - ev, key=repr)


def coverage_line(name, b: Batch, ev):
    kinds = {}
    for e in ev:
        kinds[e[0]] = kinds.get(e[0], 0) + 1
    return (f"{name}: {len(b.bufs)} blocks ({b.tags.count('filler')} fillers), {b.size} B -> K {b.K} V {b.V}; events " +
            " ".join(f"{k}:{v}" for k, v in sorted(kinds.items())))


# ------------------------------------------------------------------------------- generators
def _first(rng, kl, b):
    """A position-0 entry: key of kl bytes, empty value."""
    return (0, rb(rng, kl), b.ts(), b"")


KEY_LENS = range(1, 50)


def keys_fast(seed=501, c=C):
    """Fast path, key shapes: every (kl, p) with kl in 1..49 and p in 0..kl behind a 49-byte first
    key (s = 0 with p > 0 included), 28 shapes per block in shuffled order, once in blocks where a
    key is under 16 bytes and, for kl >= 16, once in blocks where none is (kuni; the 49-byte key has
    more pieces than the others, whose lanes repeat their clamped last piece); first keys of
    1, 15, 16, 17 and 33 bytes with p up to their length; K0 & 15 cycling over 0..15.  Values
    are 0..3 bytes.  The stream goes at all 16 leads."""
    b = Batch("keys", seed)
    rng = b.rng
    shapes = [(kl, p) for kl in KEY_LENS for p in range(kl + 1)]
    uni = [sh for sh in shapes if sh[0] >= 16]
    nb = 0
    for tag, pool in (("mixed", shapes), ("uni", uni), ("uni2", uni)):
        pool = [pool[i] for i in rng.permutation(len(pool))]
        for i in range(0, len(pool), 28):
            ents = [_first(rng, 49, b)]
            for kl, p in pool[i:i + 28]:
                ents.append((p, rb(rng, kl - p), b.ts(), rb(rng, rng.integers(0, 4))))
            b.case(block(ents), tag, kb=nb % 16)
            nb += 1
    for s0 in (1, 15, 16, 17, 33):
        ents = [_first(rng, s0, b)]
        for kl in (1, 2, s0, s0 + 1, s0 + 15, s0 + 16, 49):
            for p in range(min(kl, s0) + 1):
                if kl - p <= 49:
                    ents.append((p, rb(rng, kl - p), b.ts(), rb(rng, rng.integers(0, 4))))
        for i in range(0, len(ents) - 1, 40):
            b.case(block([ents[0]] + ents[1 + i:41 + i]), "s0", kb=nb % 16)
            nb += 1
    return b


def check_keys(ev, c=C):
    """The key generator's coverage, over the events of all 16 leads."""
    want = {("key", kl, p) for kl in KEY_LENS for p in range(kl + 1)}
    want |= {("nf", d, cls) for d in range(4) for cls in (0, 1, 2, 3, "whole")}
    want |= {("p-in-piece", x) for x in range(1, 17)}
    want |= {("key-align", u, a) for u in (False, True) for a in range(16)}
    want |= {("kuni", u, "lds") for u in (False, True)}
    want |= {("kshort", "lds", kl) for kl in range(1, 16)}
    want |= {("kshort-class", "lds", k) for k in ("1-3", "4-7", "8-15,x<4", "8-15,x>=4")}
    want |= {("kpieces", q, 4) for q in (1, 2, 3, 4)} | {("kclamp", True, a) for a in range(16)}
    want |= {("key-s0", True), ("path", "fast-lds")}
    return missing(ev, want)


VALN_NS = tuple(range(2, 65))


def values_fast(seed=502, c=C, step4=False):
    """Fast path, value shapes.
      valn     blocks of 2..64 entries (twice), values in [16, 48), 1-4-byte key suffixes; the last
               value's length chosen so that its end (the last chunk's cut) cycles over 1..16;
      off      each term that turns valn off, alone: one 15-byte value; n = 65; the output image
               over kDecOut (64 keys sharing 199 bytes: GlbSink);
      short    GlbSink blocks (three offsets to one 2000-byte value) with keys of 1..15 bytes and
               values of 0..15 bytes: every length of st_short;
      pieces   every vl in 0..48 in one block (so next to short values), ascending and shuffled,
               at each V0 & 15;
      halves   65, 100 and 128 entries (entries l and l + 64 of one lane), LdsSink and GlbSink;
      flush    every (lo, end & 15) of the value run, runs that end inside their first chunk, and
               64 * kLB whole chunks exactly, one fewer and one more.
    step4: the cut-down generator (every length a multiple of 4, as a U stream's) that must fail
    check_values."""
    b = Batch("values", seed)
    rng = b.rng

    def vlen(lo, hi):
        v = int(rng.integers(lo, hi))
        return v & ~3 if step4 else v

    nb = 0
    for rep in range(2):
        for n in VALN_NS:
            vb = (nb * 5 + nb // 16) % 16
            ents, V = [], 0
            for k in range(n):
                vl = vlen(16, 48)
                if k == n - 1 and not step4:  # the end of the last value: (vb + V + vl) & 15 cycles
                    vl = 16 + (nb % 16 - (vb + V)) % 16 + 16 * int(rng.integers(0, 2))
                sfx = rb(rng, 4 if step4 else rng.integers(1, 5))
                ents.append((0 if k == 0 else 3, sfx if k else rb(rng, 4), b.ts(), rb(rng, vl)))
                V += vl
            b.case(block(ents), "valn", vb=0 if step4 else vb)
            nb += 1
    # each term that turns valn off, alone
    ents = [(0 if k == 0 else 3, rb(rng, 4 if k == 0 else 1), b.ts(), rb(rng, 15 if k == 7 else vlen(16, 48)))
            for k in range(20)]
    b.case(block(ents), "off-short")
    ents = [(0 if k == 0 else 3, rb(rng, 4 if k == 0 else 1), b.ts(), rb(rng, vlen(16, 32))) for k in range(65)]
    b.case(block(ents), "off-n")
    ents = [(0 if k == 0 else 199, rb(rng, 200 if k == 0 else 1), b.ts(), rb(rng, vlen(16, 32))) for k in range(64)]
    b.case(block(ents), "off-sink")
    # GlbSink by value bytes (three offsets to one 2000-byte value): keys of 1..15 bytes and values of
    # 0..15 bytes go through st_short
    for rep in range(4):
        ents = [(0, rb(rng, 16), b.ts(), rb(rng, 2000))]
        for kl in range(1, 16):
            p = int(rng.integers(0, kl + 1))
            ents.append((p, rb(rng, kl - p), b.ts(), rb(rng, (kl * 7 + rep) % 16)))
        b.case(block(ents, order=[0, 0, 0] + [int(x) for x in 1 + rng.permutation(15)]), "glb-short")
    # every vl in 0..48 beside short values, at each V0 & 15
    for vb in range(16):
        for order in (np.arange(49), rng.permutation(49)):
            ents = [(0 if k == 0 else 3, rb(rng, 4 if k == 0 else 1), b.ts(), rb(rng, vl))
                    for k, vl in enumerate(order)]
            b.case(block(ents), "pieces", vb=vb)
    # entries l and l + 64
    for n in (65, 100, 128):
        for share in (3, 120):  # 128 x 121-byte keys: over kDecOut
            if share == 120 and n == 100:
                continue
            ents = [(0 if k == 0 else share, rb(rng, share + 1 if k == 0 else 1), b.ts(),
                     rb(rng, vlen(0, 16 if share == 120 else 33 if n <= 100 else 20))) for k in range(n)]
            b.case(block(ents), "halves")
    # flush edges of the value run
    for lo in range(16):
        for e in range(16):
            V = 20 + (e - lo - 20) % 16
            v0 = vlen(1, V)
            ents = [(0, rb(rng, 3), b.ts(), rb(rng, v0)), (2, rb(rng, 1), b.ts(), rb(rng, V - v0))]
            b.case(block(ents), "flush", vb=lo)
    for lo, V in ((0, 1), (0, 15), (1, 1), (1, 14), (8, 7), (14, 1), (15, 1), (15, 2)):
        b.case(block([(0, rb(rng, 5), b.ts(), rb(rng, V))]), "flush", vb=lo)
    W = 16 * 64 * c.kLB
    for lo in (0, 5):
        for V in (W - 16, W, W + 16, W + 21):
            n = 40
            ents = [(0 if k == 0 else 3, rb(rng, 4 if k == 0 else 1), b.ts(), rb(rng, int(x)))
                    for k, x in enumerate(pc._spread(V, n))]
            b.case(block(ents), "flush", kb=0, vb=lo)
    return b


def check_values(ev, c=C):
    """The value generator's coverage, over the events of the leads 0, 1, 8 and 15."""
    want = {("vpair", a, l) for a in range(16) for l in range(16)}
    want |= {("cut", x, w) for x in range(1, 17) for w in ("next", "last")}
    want |= {("a0&7", x) for x in range(8)} | {("a1&7", x) for x in range(8)}
    want |= {("lane0-chunk", a) for a in range(16)}
    want |= {("valn-n", n) for n in VALN_NS} | {("vm", m) for m in (1, 2, 3)}
    want |= {("valn-off-alone", t) for t in ("short", "n", "sink")}
    want |= {("vl", vl, a, "lds") for vl in range(49) for a in range(16)}
    want |= {("vshort", "lds", vl) for vl in range(1, 16)} | {("vempty", "lds"), ("vempty", "glb")}
    want |= {("vshort-class", s, k) for s in ("lds", "glb") for k in ("1-3", "4-7", "8-15,x<4", "8-15,x>=4")}
    want |= {("kshort", "glb", kl) for kl in range(1, 16)} | {("vshort", "glb", vl) for vl in range(1, 16)}
    want |= {("vpieces", q, 3, -(-3 // c.kLB)) for q in (1, 2, 3)} | {("vclamp", True), ("vclamp", False)}
    want |= {("second-half", s, m) for s in ("lds", "glb") for m in (1, 64)} | {("second-half", "lds", 36)}
    want |= {("flush", lo, e) for lo in range(16) for e in range(16)}
    want |= {("flush-edges", "vals", h, t, False) for h in (False, True) for t in (False, True)}
    want |= {("flush-edges", "vals", True, True, True), ("flush-edges", "vals", True, False, False)}
    want |= {("flush-whole", w) for w in ("0", "<", "=", ">")}
    want |= {("sink", "lds"), ("sink", "glb"), ("path", "fast-lds"), ("path", "fast-global")}
    return missing(ev, want)


def _mixed_entries(b, s0, n, big=0):
    """n entries behind an s0-byte first key: keys of mixed lengths and prefixes, values of mixed
    lengths; big: the length of entry 1's value (to push the block over the image)."""
    rng = b.rng
    ents = [(0, rb(rng, s0), b.ts(), rb(rng, rng.integers(0, 40)))]
    for k in range(1, n):
        kl = int(rng.integers(1, 41))
        p = int(rng.integers(0, min(kl, s0) + 1))
        ents.append((p, rb(rng, kl - p), b.ts(), rb(rng, big if k == 1 and big else rng.integers(0, 40))))
    return ents


def impossible(seed=503, c=C):
    """Valid blocks the builder cannot make ("Decode validity rules"), each as a staged
    block and as a large one (a 4200-byte value added): the offset table reversed and shuffled;
    every offset twice; gaps between the entries and before the table; the position-0 entry with
    p in 1..s0 (s0 = 24: sb < p from p = 5 + lead on) at index 0 and at index 2; on the aligned value
    path, the position-0 entry (s = 1) at index 1 of a block at stream offset 0 mod 16 behind a
    value with cut 15 (the neighbour read's least source byte, a1 = 0 at lead 0); and a large
    block of one offset that names a one-byte-key entry at the block's end (the suffix load would
    pass the block end)."""
    b = Batch("impossible", seed)
    rng = b.rng
    big_v = c.kDecImg + 72
    for big in (0, big_v):
        tag = "large-" if big else "fast-"
        for rep in range(3):
            ents = _mixed_entries(b, 24, 20, big)
            b.case(block(ents, order=range(19, -1, -1)), tag + "reversed")
            b.case(block(ents, order=rng.permutation(20)), tag + "shuffled")
            b.case(block(ents, order=rng.permutation(np.repeat(np.arange(20), 2))), tag + "aliased")
            gaps = [0] + [int(x) for x in rng.integers(0, 20, 19)]
            b.case(block(ents, order=rng.permutation(20), gaps=gaps, tailgap=int(rng.integers(1, 30))), tag + "gaps")
        for p in range(1, 25):
            for idx in (0, 2):
                ents = _mixed_entries(b, 24, 6, big)
                e0 = ents[0]
                ents[0] = (p, e0[1], e0[2], e0[3])
                order = list(range(6))
                order[0], order[idx] = order[idx], order[0]
                b.case(block(ents, order=order), tag + "p0")
    # valn: index 1 is the position-0 entry with s = 1; the value before it ends with cut 15
    for vb in range(16):
        v0 = 16 + (15 - vb - 16) % 16
        ents = [(0, rb(rng, 1), b.ts(), rb(rng, 20)), (1, rb(rng, 2), b.ts(), rb(rng, v0)),
                (0, rb(rng, 3), b.ts(), rb(rng, 33))]
        b.case(block(ents, order=[1, 0, 2]), "fast-a1", vb=vb, at=0)
    # one offset, to a 1-byte-key entry with no value at the very end of a large block
    for p, sfx in ((0, 1), (1, 0)):
        ents = [(0, rb(rng, 8), b.ts(), rb(rng, big_v)), (p, rb(rng, sfx), b.ts(), b"")]
        b.case(block(ents, order=[1]), "large-tail")
    return b


def check_impossible(ev_fast, ev_large, c=C):
    """ev_fast / ev_large: the events of the fast- and large- tagged blocks over the leads."""
    wf = {("key-bytes", i, "lds") for i in ("index0", "index>0")} | {("a1", 0), ("cut", 15, "next"), ("valn", True)}
    wf |= {("path", "fast-lds"), ("kuni", False, "lds")}
    wl = {("bkey-route", "merged"), ("bkey-route", "bytes", 0), ("bkey-route", "bytes", 1), ("path", "big-tables")}
    wl |= {("bkey-bytes-around-p", True)}
    return missing(ev_fast, wf) + missing(ev_large, wl)


def amplified(seed=504, c=C):
    """Two blocks whose decoded key bytes far exceed their own length: 128 offsets naming one
    200-byte key (GlbSink; an output sized from the input bytes is too small: the capacity retry),
    and a large block whose position-0 entry has p = s0 = 5000 (a 10000-byte key: the first-key
    load of the late pieces would pass the block end, fk + o + 16 > lim)."""
    b = Batch("amplified", seed)
    rng = b.rng
    ents = [(0, rb(rng, 200), b.ts(), rb(rng, 9)), (100, rb(rng, 100), b.ts(), rb(rng, 20))]
    b.case(block(ents, order=[1] * 64 + [0] + [1] * 63), "aliased128")
    ents = [(5000, rb(rng, 5000), b.ts(), rb(rng, 30)), (4990, rb(rng, 25), b.ts(), rb(rng, 5))]
    b.case(block(ents, order=[1, 0, 1]), "p5000")
    return b


def check_amplified(ev, b, c=C):
    want = {("sink", "glb"), ("path", "fast-global"), ("path", "big-tables"), ("bkey-route", "bytes", 2),
            ("bkey-route", "merged"), ("second-half", "glb", 64)}
    return missing(ev, want) + ([] if b.K > b.size + 16 else ["K <= input bytes + 16: no capacity retry"])


def large_totals(c=C):
    w = 64 * c.kDecBigB
    return (0, 1, 63, 64, 65, w - 1, w, w + 1)


def large_values(c=C):
    w = 16 * 64 * c.kDecBigB
    return (16, 17, 31, 32) + tuple(range(1008, 1041)) + (w - 16, w, w + 16, 65535)


LARGE_NS = (128, 129, 191, 192, 193, 256, 257)


def large(seed=505, c=C):
    """Large blocks (over kDecImg: never staged).
      keys     every (kl, p) with kl in 1..40 behind a 40-byte first key, 100 per block, beside a
               value of kDecImg + 72 bytes;
      last     two and three entries, the physically last with a value of 0..15 bytes (copy_run's
               byte loads when fewer than 16 bytes remain before the block end);
      values   16, 17, 31, 32, 1008..1040, 16 * 64 * kDecBigB -+ 16 and 65535 bytes;
      totals   128-entry blocks whose first 64 entries hold 0, 1, 63, 64, 65, 64 * kDecBigB - 1,
               64 * kDecBigB and 64 * kDecBigB + 1 pieces (the large value sits in the second 64);
      rows     a run that starts in one row of 64 pieces and ends three rows later, and runs on
               every second lane;
      counts   128, 129, 191, 192, 193, 256 and 257 tiny entries, the value before each 128-entry
               table edge long."""
    b = Batch("large", seed)
    rng = b.rng
    big_v = c.kDecImg + 72
    shapes = [(kl, p) for kl in range(1, 41) for p in range(kl + 1)]
    shapes = [shapes[i] for i in rng.permutation(len(shapes))]
    for i in range(0, len(shapes), 100):
        ents = [(0, rb(rng, 40), b.ts(), rb(rng, big_v))]
        for kl, p in shapes[i:i + 100]:
            ents.append((p, rb(rng, kl - p), b.ts(), rb(rng, rng.integers(0, 16))))
        b.case(block(ents), "keys")
    for n in (2, 3):
        for vl in range(16):
            ents = [(0, rb(rng, 6), b.ts(), rb(rng, big_v))]
            ents += [(3, rb(rng, 2), b.ts(), rb(rng, 7)) for _ in range(n - 2)]
            ents.append((3, rb(rng, 2), b.ts(), rb(rng, vl)))
            b.case(block(ents), "last")
    vals = large_values(c)
    for i in range(0, len(vals), 8):
        ents = [(0, rb(rng, 6), b.ts(), rb(rng, 3))]
        for vl in vals[i:i + 8]:
            ents.append((3, rb(rng, 2), b.ts(), rb(rng, rng.integers(0, 16))))
            ents.append((3, rb(rng, 2), b.ts(), rb(rng, vl)))
        if sum(len(e[3]) for e in ents) < big_v:
            ents.insert(1, (3, rb(rng, 2), b.ts(), rb(rng, big_v)))
        b.case(block(ents), "values")
    for total in large_totals(c):
        q = [int(x) for x in pc._spread(total, 64)]  # pieces per lane
        q = [q[i] for i in rng.permutation(64)] if total % 64 else q
        ents = []
        for k in range(128):
            vl = 16 * q[k] - int(rng.integers(0, 16)) * (q[k] > 1) if k < 64 and q[k] else int(rng.integers(0, 16))
            if k == 70:
                vl = big_v
            ents.append((0 if k == 0 else 3, rb(rng, 4 if k == 0 else 1), b.ts(), rb(rng, vl)))
        b.case(block(ents), "totals")
    # a run from row 0 into row 3; then runs on every second lane
    ents = [(0, rb(rng, 4), b.ts(), rb(rng, 16 * 40)), (3, rb(rng, 1), b.ts(), rb(rng, 16 * 200 - 5)),
            (3, rb(rng, 1), b.ts(), rb(rng, 3)), (3, rb(rng, 1), b.ts(), rb(rng, 16 * 70 + 1))]
    b.case(block(ents), "rows")
    ents = [(0 if k == 0 else 3, rb(rng, 4 if k == 0 else 1), b.ts(), rb(rng, rng.integers(16, 200) if k % 2 else k % 16))
            for k in range(64)]
    ents.append((3, rb(rng, 1), b.ts(), rb(rng, big_v)))
    b.case(block(ents), "rows")
    for n in LARGE_NS:
        ents = []
        for k in range(n):
            vl = big_v if k == 127 else 1000 if k == 255 else 0
            ents.append((0 if k == 0 else 3, rb(rng, 4 if k == 0 else 1), b.ts(), rb(rng, vl)))
        b.case(block(ents), "counts")
    return b


def check_large(ev, c=C):
    want = {("bkey", kl, p) for kl in range(1, 41) for p in range(kl + 1)}
    want |= {("bnf", d, cls) for d in range(4) for cls in (0, 1, 2, 3, "whole")}
    want |= {("bkshort", kl) for kl in range(1, 16)}
    want |= {("copy_run-short", "load16", vl) for vl in range(1, 16)}
    want |= {("copy_run-short", "bytes", vl) for vl in range(1, 10)} | {("copy_run-empty",)}
    want |= {("bvshort-class", k) for k in ("1-3", "4-7", "8-15,x<4", "8-15,x>=4")}
    want |= {("long-value", vl) for vl in large_values(c)}
    want |= {("clr-total", t) for t in large_totals(c)}
    want |= {("clr-carry", True), ("clr-carry", False), ("clr-span", 3), ("clr-span", 0), ("clr-round-span", 1)}
    want |= {("clr-holes", h) for h in ("none", "some", "many")}
    want |= {("clr-rounds", 1), ("clr-rounds", 2), ("clr-rounds-many",)} | {("clr-rows", 1), ("clr-rows", c.kDecBigB), ("clr-rows", c.kDecBigB + 1)}
    want |= {("table-chunks", n, -(-n // c.kDecMaxE), n - (n - 1) // c.kDecMaxE * c.kDecMaxE) for n in LARGE_NS if n > c.kDecMaxE}
    want |= {("long-value-before-table-edge", e) for e in (c.kDecMaxE, 2 * c.kDecMaxE)}
    want |= {("path", "big-tables"), ("path", "big-chunked"), ("bkey-route", "merged")}
    return missing(ev, want)


def simple(seed=506, c=C):
    """More than kDecMaxE tiny entries with p > 0 and empty values: 129 staged (the simple path on
    the LDS image) and 300 staged -- 300 offsets over 150 entries, as 300 entries of 16 bytes do not
    fit the image -- and both counts unstaged, which take the chunked tables."""
    b = Batch("simple", seed)
    rng = b.rng
    for n, phys, big in ((129, 129, 0), (300, 150, 0), (129, 129, c.kDecImg + 72), (300, 300, c.kDecImg + 72)):
        ents = []
        for k in range(phys):
            vl = big if k == 5 and big else 0 if k % 3 else int(rng.integers(0, 3))
            ents.append((0 if k == 0 else 2 + k % 2, rb(rng, 4 if k == 0 else k % 3 != 0), b.ts(), rb(rng, vl)))
        order = np.arange(n) % phys
        b.case(block(ents, order=order), "staged" if not big else "unstaged")
    return b


def check_simple(ev, c=C):
    want = {("simple", "lds", 129), ("simple", "lds", 300), ("simple-entry", True, False, False),
            ("simple-entry", True, True, False), ("simple-entry", True, False, True), ("path", "staged-simple"),
            ("path", "big-chunked"), ("table-chunks", 300, -(-300 // c.kDecMaxE), 300 - 299 // c.kDecMaxE * c.kDecMaxE)}
    return missing(ev, want)


GENERATORS = {"keys": keys_fast, "values": values_fast, "impossible": impossible, "amplified": amplified,
              "large": large, "simple": simple}
GEN_LEADS = {"keys": tuple(range(16)), "values": LEADS, "impossible": LEADS, "amplified": LEADS, "large": LEADS,
             "simple": LEADS}


def check(name, b: Batch, base=0, c=C):
    """The coverage of generator `name`'s batch with the stream at base + each of its leads ->
    (missing events, all events)."""
    leads = GEN_LEADS[name]
    ev = model_leads(b, leads, base, c)
    if name == "keys":
        return check_keys(ev, c), ev
    if name == "values":
        return check_values(ev, c), ev
    if name == "impossible":
        return check_impossible(model_leads(b, leads, base, c, "fast-"), model_leads(b, leads, base, c, "large-"), c), ev
    if name == "amplified":
        return check_amplified(ev, b, c), ev
    if name == "large":
        return check_large(ev, c), ev
    return check_simple(ev, c), ev
