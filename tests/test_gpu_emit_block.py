"""GPU parity of the two emit launches: emit_kernel (LSMBLK_DEBUG_EMIT_MODE 1, persistent waves
striding over the blocks) and emit_block_kernel (2, one block per single-wave workgroup in dispatch
order).  Every case runs in both modes: whichever one is the default, the other keeps its coverage,
and both must give the oracle's bytes.

Inputs and classifiers are tests/path_cases.py's; the classifiers only assert that a case reaches
the side of a threshold it was built for.  Expected bytes come from the oracle only.
"""
import functools

import numpy as np
import pytest
import torch

import path_cases as pc
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch, synth
from lsm_amd._lib import LSMBLK_DEBUG_EMIT_MODE, LSMBLK_E_CAPACITY, lib
from oracle import oracle as O
from test_gpu_parity import framed_check, seg_slots, to_dev

pytestmark = pytest.mark.gpu

MODES = [1, 2]
FILL = 0xA5
STREAM_CUS = 16  # streams A and B sized as for a 16-CU device: 36352 / >= 1536 blocks


@pytest.fixture
def emit_mode(request):
    """Sets the default-stream context's emit mode (and grid clamp) for one test."""
    ctx = batch._ctx(0)

    def set_mode(mode, clamp=0):
        assert lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_EMIT_MODE, mode | (clamp << 8)) == 0

    yield set_mode
    assert lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_EMIT_MODE, 0) == 0


@functools.lru_cache(maxsize=None)
def case_of(name):
    """(kv, seg, block_size, oracle blocks, oracle offsets) of a named case, computed once."""
    gen = {"A": lambda: pc.stream_a(STREAM_CUS), "B": lambda: pc.stream_b(STREAM_CUS),
           "count": pc.probes_emit_count, "keycap": pc.probes_emit_keycap, "valcap": pc.probes_emit_valcap,
           "sizecap": pc.probes_emit_sizecap,
           "u200": lambda: (O.KV(*synth.gen_uniform(6200, seed=61)), np.asarray([0, 2500, 6200], np.uint32), 4096)}[name]
    kv, seg, bs = gen()[:3]
    rc, ref_blocks, ref_off = O.encode_segments(kv, seg, bs)
    assert rc == 0
    for a in (ref_blocks, ref_off):
        a.setflags(write=False)
    return kv, seg, bs, ref_blocks, ref_off


def assert_bytes(got, want, ref_off, what):
    assert len(got) == len(want), what
    mism = np.flatnonzero(got != want)
    if mism.size:
        b = int(np.searchsorted(ref_off, mism[0], side="right")) - 1
        pytest.fail(f"{what}: first mismatching byte {mism[:8]} of {len(got)} (block {b} at {int(ref_off[b])})")


def packed_check(d, seg, bs, ref_blocks, ref_off, what):
    blocks, blk_off = batch.encode_kv(d, seg, bs)
    np.testing.assert_array_equal(blk_off.cpu().numpy().view(np.uint64), ref_off, err_msg=what)
    assert_bytes(blocks.cpu().numpy(), ref_blocks, ref_off, what)
    return blocks


def slot_check(kv, seg, bs, ref_blocks, ref_off, what):
    """LSMBLK_ENCODE_SEG_SLOTS through plan_walk + emit: every segment at its slot, packed == oracle."""
    out, off, so = batch.encode_kv_slots(to_dev(kv), seg, bs)
    np.testing.assert_array_equal(so[:, 0].cpu().numpy(), seg_slots(kv, seg))
    blocks, poff = batch.slots_to_packed(out, off, so)
    np.testing.assert_array_equal(poff.cpu().numpy().view(np.uint64), ref_off, err_msg=what)
    assert_bytes(blocks.cpu().numpy(), ref_blocks, ref_off, what)


def rehome(t, shift):
    """The arena at an address that is `shift` mod 16."""
    buf = torch.zeros(t.numel() + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + t.numel()] = t
    return buf[shift:shift + t.numel()]


def three_outputs(name):
    """Packed, slot and framed output of a case against the oracle -> the classification under the
    tensors' real addresses."""
    kv, seg, bs, ref_blocks, ref_off = case_of(name)
    d = to_dev(kv)
    out = packed_check(d, seg, bs, ref_blocks, ref_off, f"{name}, packed")
    slot_check(kv, seg, bs, ref_blocks, ref_off, f"{name}, slots")
    framed_check(kv, seg, bs, ref_blocks, ref_off)
    return pc.classify(ref_blocks, ref_off, kv.key_off, kv.val_off, 0, d.keys.data_ptr(), d.vals.data_ptr(),
                       out.data_ptr())


@pytest.mark.parametrize("mode", MODES)
def test_natural_packing_five_regimes(mode, emit_mode):
    """Stream B (block_size 3072; U-like, > 128 tiny entries, keys over the key cap, oversize values
    and keys): fast blocks and blocks flagged for emit_big_kernel for each reason."""
    emit_mode(mode)
    p = three_outputs("B")
    e = p.emit_counts()
    print(pc.coverage_line("B", p))
    assert e["fast"] >= 0.5 * len(p.n) and e["n"] > 0 and e["keycap"] > 0 and e["valcap"] + e["sizecap"] > 0


@pytest.mark.parametrize("edge", ["count", "keycap", "valcap", "sizecap"])
@pytest.mark.parametrize("mode", MODES)
def test_thresholds(mode, edge, emit_mode):
    """One block per segment on either side of n <= kEmitMaxE, klead + KB + 8 <= kEmitKCap, vlead + VB
    + 24 <= kEmitICap and (O & 15) + size + 8 <= kEmitICap, the arenas at every alignment mod 16."""
    emit_mode(mode)
    kv, seg, bs, ref_blocks, ref_off = case_of(edge)
    assert pc.one_block_per_segment(ref_off, seg)
    p = three_outputs(edge)
    print(pc.coverage_line("emit " + edge, p))
    if edge == "count":
        assert tuple(p.n) == pc.EMIT_COUNT_NS and pc.both_sides(p.lhs_n, pc.kEmitMaxE)
        np.testing.assert_array_equal(p.fail, np.where(p.n > pc.kEmitMaxE, pc.FAIL_N, 0))
        return
    seen_k, lv, ls, leads = {}, set(), set(), set()
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
        leads |= set(zip(q.klead.tolist(), q.vlead.tolist(), q.olead.tolist()))
    icap = set(range(pc.kEmitICap - 17, pc.kEmitICap + 18))
    if edge == "keycap":
        for kl in range(16):
            assert {pc.kEmitKCap, pc.kEmitKCap + 1} <= seen_k[kl], kl
    elif edge == "valcap":
        assert icap <= lv and icap <= ls
        assert {v for _, v, _ in leads} == set(range(16)) and {o for _, _, o in leads} == set(range(16))
    else:
        assert icap <= ls and ((p.fail & ~pc.FAIL_S) == 0).all()
        assert {v for _, v, _ in leads} == set(range(16))


@pytest.mark.parametrize("mode", MODES)
def test_fast_and_big_blocks_interleaved(mode, emit_mode):
    """Stream A: one entry per block, single big blocks between fast ones everywhere and a region
    where 30 % are big, the first and the last block big."""
    emit_mode(mode)
    kv, seg, bs, ref_blocks, ref_off = case_of("A")
    d = to_dev(kv)
    out = packed_check(d, seg, bs, ref_blocks, ref_off, "A, packed")
    slot_check(kv, seg, bs, ref_blocks, ref_off, "A, slots")
    p = pc.classify(ref_blocks, ref_off, kv.key_off, kv.val_off, 0, d.keys.data_ptr(), d.vals.data_ptr(), out.data_ptr())
    assert (p.n == 1).all()
    order = pc.wave_sequences(p.is_big, 1)[0]  # the blocks in dispatch order
    assert order.startswith("BF") and order.endswith("FB")
    for pat in ("FBF", "FBBF", "FBBBF"):
        assert pat in order, pat
    e = p.emit_counts()
    assert e["keycap"] > 0 and e["valcap"] > 0 and e["fast"] > 0


def raw_encode(d, seg, bs, out_cap, blk_cap, out=None):
    """One lsmblk_encode_batch call with the caller's capacities -> (status, stats, out, blk_off)."""
    if out is None:
        out = batch._aligned_empty(max(out_cap, 16), "cuda")
    off = torch.zeros(max(blk_cap, 1), dtype=torch.int64, device="cuda")
    st = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device="cuda")
    seg_t = torch.from_numpy(np.asarray(seg, np.int64).astype(np.uint32).view(np.int32)).cuda()
    batch.encode_into(d, seg_t, len(seg) - 1, bs, out, out_cap, off, blk_cap, st)
    torch.cuda.synchronize()
    return batch._status(st), st.cpu().tolist(), out, off


@pytest.mark.parametrize("mode", MODES)
def test_grid_edges(mode, emit_mode):
    """blk_cap exactly the offsets the blocks need, one more, and the loose entries + 2 (most
    workgroups of the per-block grid find no block); the grid clamped to 64 workgroups over 200
    blocks (every workgroup loops over three or four blocks); one block; no entries in one empty
    segment; a segment of one entry."""
    kv, seg, bs, ref_blocks, ref_off = case_of("u200")
    nblk = len(ref_off) - 1
    assert 190 <= nblk <= 210
    d = to_dev(kv)
    cap = len(ref_blocks) + 16
    for clamp in (0, 64):
        emit_mode(mode, clamp)
        for blk_cap in (nblk + 1, nblk + 2, kv.n + 2):
            status, st, out, off = raw_encode(d, seg, bs, cap, blk_cap)
            what = f"blk_cap {blk_cap}, clamp {clamp}"
            assert status == 0 and st[0] == nblk and st[1] == len(ref_blocks), what
            np.testing.assert_array_equal(off[:nblk + 1].cpu().numpy().view(np.uint64), ref_off, err_msg=what)
            assert_bytes(out[:len(ref_blocks)].cpu().numpy(), ref_blocks, ref_off, what)
    emit_mode(mode)
    one = O.KV(*synth.gen_uniform(20, seed=62))
    for small, sseg in ((one, [0, one.n]), (one, [0, 1, one.n]), (one, [0, one.n - 1, one.n])):
        rc, want, want_off = O.encode_segments(small, sseg, 4096)
        assert rc == 0 and len(want_off) - 1 == len(sseg) - 1
        packed_check(to_dev(small), sseg, 4096, want, want_off, f"segments {sseg}")
    empty = O.KV.from_entries([])
    status, st, out, off = raw_encode(to_dev(empty), [0, 0], 4096, 16, 2)
    assert status == 0 and st[0] == 0 and st[1] == 0 and int(off[0].item()) == 0


@pytest.mark.parametrize("mode", MODES)
def test_capacity_one_byte_short_of_the_last_block(mode, emit_mode):
    """out_cap one byte short of the last block: LSMBLK_E_CAPACITY, every earlier block byte-exact,
    the bytes from the last block's start on keep their fill."""
    emit_mode(mode)
    kv, seg, bs, ref_blocks, ref_off = case_of("u200")
    total, last = int(ref_off[-1]), int(ref_off[-2])
    out = batch._aligned_empty(total + 64, "cuda")
    out.fill_(FILL)
    status, st, out, off = raw_encode(to_dev(kv), seg, bs, total - 1, kv.n + 2, out=out)
    assert status == LSMBLK_E_CAPACITY
    got = out.cpu().numpy()
    assert_bytes(got[:last], ref_blocks[:last], ref_off, "blocks before the last")
    assert (got[last:] == FILL).all(), "bytes past the last written block changed"


def test_compaction_reads_n_from_the_device(emit_mode):
    """lsmblk_compact_batch through compact_into in mode 2: the encode's entry count and segment
    table come from device memory, blk_cap is the loose entries + 2."""
    emit_mode(2)
    keys, ko, vals, vo, ts, rs = synth.gen_runs(4000, nrun=3, seed=63, versions=2, tombstone=0.1)
    kv = O.KV(keys, ko, vals, vo, ts)
    wm, bs, target = int(int(ts.max()) * 0.5), 4096, 64 << 10
    src = O.merge_runs(kv, rs)
    want = O.compact(kv, src, wm, True, (), bs, target)
    d = to_dev(kv)
    dev = torch.device("cuda", 0)
    rst = batch._u32_table(rs, dev)
    kb, vb = d.byte_sizes()
    buf = batch.CompactBuffers(d.n, kb, vb, dev, target_sst_size=target)
    batch.compact_into(d, rst, rst.numel() - 1, batch.compact_opts(wm, True, (), bs, target, dev), buf)
    torch.cuda.synchronize()
    assert batch._status(buf.stats) == 0
    s = buf.stats.cpu().tolist()
    nblk, nbytes = s[0], s[1]
    assert nblk == len(want["blk_off"]) - 1 and nblk > 8 and len(want["sst_blk"]) > 2
    np.testing.assert_array_equal(buf.blk_off[:nblk + 1].cpu().numpy().view(np.uint64), want["blk_off"])
    assert_bytes(buf.out[:nbytes].cpu().numpy(), want["blocks"], want["blk_off"], "compaction blocks")
