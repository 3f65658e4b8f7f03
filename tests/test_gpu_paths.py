"""GPU parity on the paths no other input reaches: the persistent emit loops (emit_kernel, fuse_emit)
walking mixed sequences of fast and big blocks inside one wave, emit_big_kernel's second ballot
round, blocks on either side of every predicate that picks a decode or emit path, and block
counts on the lagged decode's tile edges.

The inputs and the coverage conditions are tests/path_cases.py's (checked on the CPU by
test_path_cases.py); the conditions are asserted again here for the device's CU count and the
tensors' real addresses.  Expected bytes and streams come from the oracle only.
"""
import numpy as np
import pytest
import torch

import path_cases as pc
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch, synth
from lsm_amd._lib import LSMBLK_DEBUG_DECODE_LAG, LSMBLK_DEBUG_TWO_PASS_DECODE
from oracle import oracle as O
from test_gpu_parity import assert_kv_equal, dev_blocks, framed_check, framed_want, slot_check, to_dev

pytestmark = pytest.mark.gpu


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def oracle_of(case):
    kv, seg, bs = case[:3]
    rc, ref_blocks, ref_off = O.encode_segments(kv, seg, bs)
    assert rc == 0
    rc, ref_kv = O.decode_blocks(ref_blocks, ref_off)
    assert rc == 0 and pc.kv_equal(ref_kv, kv)
    return ref_blocks, ref_off, ref_kv


def packed_check(d, seg, bs, ref_blocks, ref_off, what=""):
    """The packed encode == the oracle's offsets and bytes -> the output tensor."""
    blocks, blk_off = batch.encode_kv(d, seg, bs)
    np.testing.assert_array_equal(blk_off.cpu().numpy().view(np.uint64), ref_off, err_msg=what)
    got = blocks.cpu().numpy()
    assert len(got) == len(ref_blocks), what
    mism = np.flatnonzero(got != ref_blocks)
    if mism.size:
        b = int(np.searchsorted(ref_off, mism[0], side="right")) - 1
        pytest.fail(f"{what}: first mismatching byte {mism[:8]} of {len(got)} (block {b} at {int(ref_off[b])})")
    return blocks


def decode_check(ref_blocks, ref_off, ref_kv, shift=0, what=""):
    """The GPU decode of the oracle's blocks == the oracle's decode, with the block entry index."""
    db, do = dev_blocks(ref_blocks, ref_off, shift)
    dkv, ent = batch.decode_blocks(db, do, with_blk_ent=True)
    assert_kv_equal(dkv, ref_kv)
    counts = pc.block_entry_counts(ref_blocks, ref_off)
    np.testing.assert_array_equal(ent.cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]), err_msg=what)
    return db


def full_check(kv, seg, bs, ref_blocks, ref_off, ref_kv):
    """Packed encode (twice on the context: the epoch advances), slot encode unfused and fused,
    framed encode, decode -> the path classification under the tensors' real addresses."""
    d = to_dev(kv)
    packed_check(d, seg, bs, ref_blocks, ref_off, "packed")
    out = packed_check(d, seg, bs, ref_blocks, ref_off, "packed, second call")
    slot_check(kv, seg, bs, ref_blocks, ref_off)
    framed_check(kv, seg, bs, ref_blocks, ref_off)
    db = decode_check(ref_blocks, ref_off, ref_kv)
    return pc.classify(ref_blocks, ref_off, kv.key_off, kv.val_off, db.data_ptr(), d.keys.data_ptr(),
                       d.vals.data_ptr(), out.data_ptr())


def rehome(t, shift):
    """The arena at an address that is `shift` mod 16."""
    buf = torch.zeros(t.numel() + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + t.numel()] = t
    return buf[shift:shift + t.numel()]


@pytest.mark.parametrize("which", ["A", "B"])
def test_emit_wave_loops_mixed_paths(which):
    """Stream A (71 one-entry blocks per wave at 32 waves per CU; 0.2 % big blocks, 30 % in one
    region, the first and the last block big) and stream B (natural packing over five regimes at
    block_size 3072): every wave of emit_kernel / fuse_emit walks fast and flagged blocks in turn,
    emit_big_kernel ballots a second round of candidates (A)."""
    cus = cu_count()
    case = pc.stream_a(cus) if which == "A" else pc.stream_b(cus)
    kv, seg, bs = case
    ref_blocks, ref_off, ref_kv = oracle_of(case)
    p = full_check(kv, seg, bs, ref_blocks, ref_off, ref_kv)
    (pc.check_stream_a if which == "A" else pc.check_stream_b)(p, cus)
    print(f"{cus} CUs; " + pc.coverage_line(which, p))


def _probe_case(case):
    kv, seg, bs = case[:3]
    ref_blocks, ref_off, ref_kv = oracle_of(case)
    assert pc.one_block_per_segment(ref_off, seg)
    return kv, seg, bs, ref_blocks, ref_off, ref_kv


@pytest.mark.parametrize("edge", ["count", "keycap", "valcap", "sizecap"])
def test_emit_dispatch_edges(edge):
    """One block per segment on either side of emit's predicates: n <= kEmitMaxE, klead + KB + 8 <=
    kEmitKCap, vlead + VB + 24 <= kEmitICap, (O & 15) + size + 8 <= kEmitICap -- the key and value
    arenas at every alignment mod 16."""
    gen = {"count": pc.probes_emit_count, "keycap": pc.probes_emit_keycap, "valcap": pc.probes_emit_valcap,
           "sizecap": pc.probes_emit_sizecap}[edge]
    kv, seg, bs, ref_blocks, ref_off, ref_kv = _probe_case(gen())
    p = full_check(kv, seg, bs, ref_blocks, ref_off, ref_kv)
    print(pc.coverage_line("emit " + edge, p))
    if edge == "count":
        assert tuple(p.n) == pc.EMIT_COUNT_NS and pc.both_sides(p.lhs_n, pc.kEmitMaxE)
        np.testing.assert_array_equal(p.fail, np.where(p.n > pc.kEmitMaxE, pc.FAIL_N, 0))
        return
    seen_k, lv, ls, alone = {}, set(), set(), 0
    for shift in range(16):
        d = to_dev(kv)
        if edge == "keycap":
            d.keys = rehome(d.keys, shift)
        else:
            d.vals = rehome(d.vals, shift)
        out = packed_check(d, seg, bs, ref_blocks, ref_off, f"{edge}, arena at {shift} mod 16")
        q = pc.classify(ref_blocks, ref_off, kv.key_off, kv.val_off, 0, d.keys.data_ptr(), d.vals.data_ptr(),
                        out.data_ptr())
        for kl, lhs in zip(q.klead, q.lhs_k):
            seen_k.setdefault(int(kl), set()).add(int(lhs))
        lv |= set(q.lhs_v.tolist())
        ls |= set(q.lhs_s.tolist())
        alone += int(((q.fail == pc.FAIL_V) & (q.vlead >= q.olead + 4)).sum())
    icap = set(range(pc.kEmitICap - 17, pc.kEmitICap + 18))
    if edge == "keycap":
        for kl in range(16):
            assert {pc.kEmitKCap, pc.kEmitKCap + 1} <= seen_k[kl], kl
    elif edge == "valcap":
        assert icap <= lv and icap <= ls
        assert alone > 0, "no block where the value cap fails and the size cap holds"
    else:
        assert icap <= ls and ((p.fail & ~pc.FAIL_S) == 0).all() and max(lv) <= pc.kEmitICap - 1000


@pytest.mark.parametrize("edge", ["staged", "count", "outimage"])
def test_decode_dispatch_edges(edge):
    """One block per segment on either side of the decode's predicates: lead + len + 15 <= kDecImg
    (the block stream at every alignment mod 16), n <= kDecMaxE staged and unstaged, and the LDS
    output image ((kb + K + 15) & ~15) + ((vb + V + 15) & ~15) <= kDecOut for the output offsets'
    low bits (kb, vb) in {0, 1, 8, 15}^2."""
    gen = {"staged": pc.probes_dec_staged, "count": pc.probes_dec_count, "outimage": pc.probes_dec_outimage}[edge]
    case = gen()
    kv, seg, bs, ref_blocks, ref_off, ref_kv = _probe_case(case)
    p = full_check(kv, seg, bs, ref_blocks, ref_off, ref_kv)
    print(pc.coverage_line("decode " + edge, p))
    if edge == "staged":
        ln = np.diff(ref_off.astype(np.int64))
        seen = {}
        for shift in range(16):
            db = decode_check(ref_blocks, ref_off, ref_kv, shift, f"block stream at {shift} mod 16")
            q = pc.classify(ref_blocks, ref_off, kv.key_off, kv.val_off, db.data_ptr())
            for n, ld, lhs in zip(q.n, q.lhs_img - ln - 15, q.lhs_img):
                seen.setdefault((int(n), int(ld)), set()).add(int(lhs))
        for n in (1, 2, 128):
            for ld in range(16):
                assert {pc.kDecImg, pc.kDecImg + 1} <= seen[(n, ld)], (n, ld)
    elif edge == "count":
        nstaged = case[3]
        small = p.n <= pc.kDecMaxE
        want = np.where(np.arange(len(p.n)) < nstaged, np.where(small, 0, 2), np.where(small, 3, 4))
        np.testing.assert_array_equal(p.dec, want)
        assert tuple(p.n[nstaged:]) == pc.DEC_COUNT_NS
        assert sorted(p.n[:nstaged]) == [n for n in pc.DEC_COUNT_NS if n <= pc.DEC_COUNT_STAGED_MAX]
        decode_check(ref_blocks, ref_off, ref_kv, 5)
    else:
        m = p.n == 30
        for kb in pc.OUT_LEADS:
            for vb in pc.OUT_LEADS:
                q = m & (p.kb == kb) & (p.vb == vb)
                assert pc.both_sides(p.lhs_out[q], pc.kDecOut, near=16) and {0, 1} <= set(p.dec[q]), (kb, vb)
        decode_check(ref_blocks, ref_off, ref_kv, 5)


TILE_EDGE_NBLK = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 511, 512, 513, 575, 576, 577)


def test_decode_block_counts_on_tile_edges():
    """The first nblk blocks of a U stream for nblk on the edges of the 64-block count tiles (and of
    the 8-tile rotation of the finisher workgroups): the lagged decode at its default lag and at
    the smallest (128, which the host raises to for short batches), the two-pass decode, and the
    CRC-verifying framed read -- stream and block entry index against the oracle."""
    from lsm_amd._lib import lib
    kv = O.KV(*synth.gen_uniform(18500, seed=41))
    rc, ref_blocks, ref_off = O.encode_segments(kv, [0, kv.n], 4096)
    assert rc == 0 and len(ref_off) - 1 >= max(TILE_EDGE_NBLK)
    rc, ref_kv = O.decode_blocks(ref_blocks, ref_off)
    assert rc == 0
    ent = np.concatenate([[0], np.cumsum(pc.block_entry_counts(ref_blocks, ref_off))])
    ctx = batch._ctx(0)
    try:
        for mode in ("default", "lag128", "two_pass", "framed"):
            assert lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_TWO_PASS_DECODE, int(mode == "two_pass")) == 0
            assert lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_DECODE_LAG, 128 if mode == "lag128" else 0) == 0
            for nblk in TILE_EDGE_NBLK:
                e, end = int(ent[nblk]), int(ref_off[nblk])
                want = O.KV(ref_kv.keys[:ref_kv.key_off[e]], ref_kv.key_off[:e + 1], ref_kv.vals[:ref_kv.val_off[e]],
                            ref_kv.val_off[:e + 1], ref_kv.ts[:e])
                if mode == "framed":
                    data, off = framed_want(ref_blocks[:end], ref_off[:nblk + 1])
                    db, do = dev_blocks(np.frombuffer(data, np.uint8).copy(), off, 3)
                    got, gent = batch.decode_blocks(db, do, tail=4, verify=True, with_blk_ent=True)
                else:
                    db, do = dev_blocks(ref_blocks[:end], ref_off[:nblk + 1])
                    got, gent = batch.decode_blocks(db, do, with_blk_ent=True)
                assert got.n == e, (mode, nblk)
                assert_kv_equal(got, want)
                np.testing.assert_array_equal(gent.cpu().numpy(), ent[:nblk + 1], err_msg=f"{mode}, {nblk} blocks")
    finally:
        lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_TWO_PASS_DECODE, 0)
        lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_DECODE_LAG, 0)
