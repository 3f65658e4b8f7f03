"""Blocks for the decode's in-place value compaction (dec_fast_outputs in lsmblk_gpu.hip) -- TEST
INFRASTRUCTURE, shared by test_decode_inplace_cases.py (CPU) and test_gpu_decode_inplace.py (GPU).

  constants   kDecKeyImg (the key image), kDecMB (chunk groups per move batch) and kDecMapN read out
              of the source beside decode_cases.C (kDecImg, kDecMaxE, kDecOut).
  route()     a plain restatement of which route a block takes at a given address and output
              base, and the figures the cases are named for (whole chunks, d_0, the key run).  It is
              never the expected output, which is the C oracle's decode.
  cases       CASES: name -> builder of a decode_cases.Batch.  Blocks come from the oracle's block
              builder; only the blocks no encoder writes (an offsets table out of order, an entry
              named twice, gaps) are assembled by decode_cases.block.  A block under test follows a
              one-entry filler block whose value bytes set V0 & 15 and whose length sets the
              block's address & 15 (the stream itself is placed at a 16-B-aligned address).
"""
import numpy as np

import decode_cases as dc
import path_cases as pc
from oracle import oracle as O

_K = pc.read_constants(dc.GPU_SRC, ("kDecKeyImg", "kDecMB", "kDecMapN"))
kDecKeyImg, kDecMB, kDecMapN = _K["kDecKeyImg"], _K["kDecMB"], _K["kDecMapN"]
kDecImg, kDecMaxE, kDecOut = dc.C.kDecImg, dc.C.kDecMaxE, dc.C.kDecOut
BATCH = 64 * kDecMB  # destination chunks per move batch

VLENS = (16, 17, 31, 32, 33, 100, 15)
COUNTS = (1, 2, 63, 64, 65, 128, 129)


def route(buf, lead, K0, V0):
    """-> (route, info).  route: 'inplace', 'glb:order' / 'glb:keys' / 'glb:out' (the GlbSink
    fallbacks, in the kernel's order of tests), 'simple' (over kDecMaxE entries) or 'big' (over the
    image).  info: n, kb, vb, K, V, krun, whole (chunks below it can be moved), moved (chunks lying
    wholly inside one value), d0, short (values under 16 B), zero (empty values)."""
    n, _, _, ents = dc.parse(buf)
    kb, vb = K0 & 15, V0 & 15
    K, V = sum(p + s for _, p, s, _ in ents), sum(vl for _, _, _, vl in ents)
    vout = np.concatenate([[0], np.cumsum([vl for _, _, _, vl in ents])])
    d = [lead + off + 14 + s - (vb + int(vout[k])) for k, (off, _, s, _) in enumerate(ents)]
    krun = (kb + K + 15) & ~15
    moved = sum(max((vb + int(vout[k]) + vl) // 16 - (vb + int(vout[k]) + 15) // 16, 0) for k, (_, _, _, vl) in enumerate(ents))
    info = dict(lead=lead, n=n, kb=kb, vb=vb, K=K, V=V, krun=krun, whole=(vb + V) >> 4, moved=moved, d0=d[0],
                short=sum(0 < vl < 16 for _, _, _, vl in ents), zero=sum(vl == 0 for _, _, _, vl in ents),
                first_s=ents[0][2])
    if lead + len(buf) + 15 > kDecImg:
        return "big", info
    if n > kDecMaxE:
        return "simple", info
    if d[0] < 0 or any(y < x for x, y in zip(d, d[1:])):
        return "glb:order", info
    if krun > kDecKeyImg:
        return "glb:keys", info
    if krun + ((vb + V + 15) & ~15) > kDecOut:
        return "glb:out", info
    return "inplace", info


def routes(b, base=0):
    """[(tag, route, info)] of a Batch whose stream starts at address `base`."""
    out, pos = [], base
    for buf, tag, K0, V0 in zip(b.bufs, b.tags, b.K0, b.V0):
        out.append((tag,) + route(buf, pos & 15, K0, V0))
        pos += len(buf)
    return out


def enc(entries):
    """One block of [(key, ts, value)] from the oracle's block builder."""
    bld = O.Builder(1 << 16)
    for k, t, v in entries:
        assert bld.add(k, t, v) == 1
    return bld.finish()


def keys_of(rng, n, klen, shared=0):
    """n ascending keys of klen bytes (klen >= 1) sharing their first `shared` bytes."""
    head = dc.rb(rng, shared)
    if klen - shared >= 2:
        return [head + dc.rb(rng, klen - shared - 2) + bytes([1 + i // 200, 1 + i % 200]) for i in range(n)]
    assert n <= 200 and klen - shared == 1
    return [head + bytes([1 + i]) for i in range(n)]


def blk(b, vlens, klen=12, shared=0, keys=None):
    keys = keys or keys_of(b.rng, len(vlens), klen, shared)
    return enc([(k, b.ts(), dc.rb(b.rng, vl)) for k, vl in zip(keys, vlens)])


# ------------------------------------------------------------------------------- the cases
def align():
    """Every (lead, V0 & 15): a 6-entry block with values on both sides of 16 bytes."""
    b = dc.Batch("align", 501)
    for lead in range(16):
        for vb in range(16):
            b.case(blk(b, (40, 16, 15, 33, 100, 17)), f"align:{lead}:{vb}", vb=vb, at=lead)
    return b


def vlens():
    """Every value length of VLENS first, in the middle and last among 40-byte values."""
    b = dc.Batch("vlens", 502)
    for vl in VLENS:
        for pos in (0, 2, 4):
            v = [40] * 5
            v[pos] = vl
            b.case(blk(b, v), f"vlen:{vl}:{pos}")
    return b


def first_keys():
    """A one-byte first key at lead 0 under every V0 & 15 (15: d_0 = 0, the tight case), and first
    keys that fill the key image exactly, one byte under and one over, alone in their block."""
    b = dc.Batch("first_keys", 503)
    for vb in range(16):
        b.case(blk(b, (37, 16, 64), keys=[b"\x05", b"\x05\x01", b"\x06"]), f"first1:{vb}", vb=vb, at=0)
        b.case(blk(b, (70,), keys=[b"\x07"]), f"first1-alone:{vb}", vb=vb, at=0)
    for kb in (0, 7, 15):
        for over in (-1, 0, 1):
            b.case(blk(b, (100,), klen=kDecKeyImg - kb + over), f"firstmax:{kb}:{over}", kb=kb)
    return b


def key_image():
    """16 keys sharing 100 bytes whose run ends 17 and 1 bytes under the key image's end, at it, and
    1 byte past it (the GlbSink), at three K0 & 15."""
    b = dc.Batch("key_image", 504)
    for kb in (0, 3, 15):
        for over in (-17, -1, 0, 1):
            total = kDecKeyImg - kb + over
            klen, extra = divmod(total, 16)
            ks = keys_of(b.rng, 16, klen, 100)
            ks[-1] = ks[-1] + bytes([9]) * extra
            b.case(blk(b, [24] * 16, keys=ks), f"keyimg:{kb}:{over}", kb=kb)
    return b


def out_bound():
    """Key run + value run in whole chunks at kDecOut exactly, one value byte under the last chunk's
    end, and one byte over (the GlbSink): 20 keys of 100 bytes sharing 96."""
    b = dc.Batch("out_bound", 505)
    for kb, vb in ((0, 0), (5, 15), (15, 1)):
        for over in (-1, 0, 1):
            krun = (kb + 2000 + 15) & ~15
            V = kDecOut - krun - vb + over
            v = [V // 20] * 20
            v[-1] += V - sum(v)
            b.case(blk(b, v, klen=100, shared=96), f"out:{kb}:{vb}:{over}", kb=kb, vb=vb)
    return b


def counts():
    """1, 2, 63, 64, 65, 128 and 129 entries (129: the simple path), values of 16 bytes and more
    mixed with shorter ones so that the block stays inside the image."""
    b = dc.Batch("counts", 506)
    for n in COUNTS:
        for rep in range(2):
            room = 3900 - 20 * n
            long_ = max(1, min(n, room // 48)) if n <= 65 else 24
            v = [int(x) for x in b.rng.integers(16, 40, long_)] + [int(x) for x in b.rng.integers(1, 9, n - long_)]
            b.rng.shuffle(v)
            b.case(blk(b, v, klen=4, shared=2), f"count:{n}:{rep}")
    return b


def batches():
    """Value runs of exactly BATCH / 2, BATCH and 2 BATCH whole chunks and one chunk more: the move
    loop's group and batch boundaries."""
    b = dc.Batch("batches", 507)
    for nw in (BATCH // 2, BATCH // 2 + 1, BATCH, BATCH + 1):
        for vb, rest in ((0, 0), (9, 15), (15, 3)):
            V = 16 * nw - vb + rest
            v = [V // 12] * 12
            v[0] += V - sum(v)
            b.case(blk(b, v), f"batch:{nw}:{vb}", vb=vb)
    return b


def overlap():
    """200 blocks of mixed shapes back to back, no fillers: neighbours share 16-B chunks and 128-B
    lines in the key and value arenas, so a store past a block's own bytes lands in a neighbour's."""
    b = dc.Batch("overlap", 508)
    for i in range(200):
        n = int(b.rng.integers(1, 40))
        kind = int(b.rng.integers(4))
        if kind == 0:
            v = [int(x) for x in b.rng.integers(0, 16, n)]
        elif kind == 1:
            v = [int(x) for x in b.rng.integers(16, 90, n)]
        else:
            v = [int(x) for x in b.rng.choice((0, 1, 7, 15, 16, 17, 31, 32, 33, 64, 100), n)]
        klen = int(b.rng.integers(3, 40))
        while sum(v) + len(v) * (16 + klen) + 2 > 3900:  # stay inside the image
            v.pop()
        b.add(blk(b, v, klen=klen, shared=int(b.rng.integers(0, klen - 1))), f"mix:{i}")
    return b


def order():
    """Well-formed blocks no encoder writes: the offsets table backwards, one entry named twice and
    values amplified past the block (the GlbSink: nothing may be compacted over an unread source),
    and entries in order with gaps between them (in place: d grows by more than a header)."""
    b = dc.Batch("order", 509)
    rng = b.rng

    def ents(n, vl):
        ks = keys_of(rng, n, 10)
        return [(0, ks[i], b.ts(), dc.rb(rng, vl)) for i in range(n)]
    for vb in (0, 15):
        b.case(dc.block(ents(6, 40), order=[5, 4, 3, 2, 1, 0]), "order:reversed", vb=vb, at=0)
        b.case(dc.block(ents(6, 40), order=[0, 1, 3, 2, 4, 5]), "order:swap", vb=vb, at=3)
        b.case(dc.block(ents(4, 48), order=[0, 1, 1, 2, 3]), "order:twice", vb=vb, at=9)
        b.case(dc.block(ents(3, 200), order=[0, 1, 2] + [2] * 12), "order:amplified", vb=vb)
        b.case(dc.block(ents(5, 33), gaps=[0, 1, 15, 16, 40], tailgap=7), "order:gaps", vb=vb, at=0)
    return b


CASES = {"align": align, "vlens": vlens, "first_keys": first_keys, "key_image": key_image, "out_bound": out_bound,
         "counts": counts, "batches": batches, "overlap": overlap, "order": order}
