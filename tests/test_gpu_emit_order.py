"""GPU parity of emit_block_kernel's block order: within every whole group of 64 consecutive
workgroups, workgroup t takes the group's block 8 (t mod 8) + t / 8; a partial last group keeps the
identity; the same at every stride of a clamped grid.  A block emitted twice or never shows as wrong
bytes against the oracle (the output starts from a fill pattern) -- so the cases sit on the edges of
the groups: 1, 7, 8, 9, 63, 64, 65, 127, 128, 129 and 200 blocks, under a grid of exactly the blocks
+ 1 (tight blk_cap), of the loose entries + 2, and clamped to 64 and to 72 workgroups.

Every case runs in emit modes 1 (emit_kernel) and 2 (emit_block_kernel), packed, in slots and
framed: whichever kernel is not the default keeps its coverage.  Expected bytes come from the
oracle only.
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
NBLK = [1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200]
FILL = 0xA5


@pytest.fixture
def emit_mode():
    """Sets the default-stream context's emit mode (and grid clamp) for one test."""
    ctx = batch._ctx(0)

    def set_mode(mode, clamp=0):
        assert lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_EMIT_MODE, mode | (clamp << 8)) == 0

    yield set_mode
    assert lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_EMIT_MODE, 0) == 0


def head(kv, n):
    """The stream's first n entries."""
    return O.KV(kv.keys[:int(kv.key_off[n])].copy(), kv.key_off[:n + 1].copy(), kv.vals[:int(kv.val_off[n])].copy(),
                kv.val_off[:n + 1].copy(), kv.ts[:n].copy())


@functools.lru_cache(maxsize=None)
def stream():
    """A U stream of a little over 200 blocks in one segment -> (kv, first entry of every block)."""
    kv = O.KV(*synth.gen_uniform(6600, seed=71))
    rc, blocks, off = O.encode_segments(kv, [0, kv.n], 4096)
    assert rc == 0 and len(off) - 1 > 202
    first = np.concatenate([[0], np.cumsum(pc.block_entry_counts(blocks, off.astype(np.int64)))])
    return kv, first


def oracle_of(kv, seg):
    rc, ref_blocks, ref_off = O.encode_segments(kv, seg, 4096)
    assert rc == 0
    for a in (ref_blocks, ref_off):
        a.setflags(write=False)
    return kv, np.asarray(seg, np.uint32), ref_blocks, ref_off


@functools.lru_cache(maxsize=None)
def case_of(nblk):
    """Exactly nblk blocks over three segments, cut at block starts (the greedy packing restarts the
    same way there); the one-block case has an empty segment on either side of its block."""
    kv, first = stream()
    a, b = int(first[nblk // 3]), int(first[(2 * nblk + 2) // 3])
    c = oracle_of(head(kv, int(first[nblk])), [0, a, b, int(first[nblk])])
    assert len(c[3]) - 1 == nblk
    return c


@functools.lru_cache(maxsize=None)
def case_edge_segments():
    """~200 blocks with an empty and a one-entry segment in the middle."""
    kv, first = stream()
    m = int(first[100])
    c = oracle_of(head(kv, int(first[200])), [0, m, m, m + 1, int(first[200])])
    assert 200 <= len(c[3]) - 1 <= 202
    return c


def assert_bytes(got, want, ref_off, what):
    assert len(got) == len(want), what
    mism = np.flatnonzero(got != want)
    if mism.size:
        b = int(np.searchsorted(ref_off, mism[0], side="right")) - 1
        pytest.fail(f"{what}: first mismatching byte {mism[:8]} of {len(got)} (block {b} at {int(ref_off[b])})")


def raw_encode(d, seg, out_cap, blk_cap, total):
    """One lsmblk_encode_batch call into a filled buffer -> (status, stats, out, blk_off)."""
    out = batch._aligned_empty(total + 64, "cuda")
    out.fill_(FILL)
    off = torch.zeros(max(blk_cap, 1), dtype=torch.int64, device="cuda")
    st = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device="cuda")
    seg_t = torch.from_numpy(np.asarray(seg, np.int64).astype(np.uint32).view(np.int32)).cuda()
    batch.encode_into(d, seg_t, len(seg) - 1, 4096, out, out_cap, off, blk_cap, st)
    torch.cuda.synchronize()
    return batch._status(st), st.cpu().tolist(), out.cpu().numpy(), off


def packed_raw(case, blk_cap, what):
    """Packed output under the caller's blk_cap: stats[0] == nblk, offsets, every block's bytes, and
    nothing written past the last block."""
    kv, seg, ref_blocks, ref_off = case
    nblk, total = len(ref_off) - 1, len(ref_blocks)
    status, st, got, off = raw_encode(to_dev(kv), seg, total + 16, blk_cap, total)
    assert status == 0 and st[0] == nblk and st[1] == total, what
    np.testing.assert_array_equal(off[:nblk + 1].cpu().numpy().view(np.uint64), ref_off, err_msg=what)
    assert_bytes(got[:total], ref_blocks, ref_off, what)
    assert (got[total:] == FILL).all(), what + ": bytes past the last block changed"


def slots(case, what):
    """LSMBLK_ENCODE_SEG_SLOTS through plan_walk + emit: every segment at its slot, packed == oracle."""
    kv, seg, ref_blocks, ref_off = case
    out, off, so = batch.encode_kv_slots(to_dev(kv), seg, 4096)
    np.testing.assert_array_equal(so[:, 0].cpu().numpy(), seg_slots(kv, seg))
    blocks, poff = batch.slots_to_packed(out, off, so)
    np.testing.assert_array_equal(poff.cpu().numpy().view(np.uint64), ref_off, err_msg=what)
    assert_bytes(blocks.cpu().numpy(), ref_blocks, ref_off, what)


def three_outputs(case, what):
    kv, seg, ref_blocks, ref_off = case
    nblk = len(ref_off) - 1
    packed_raw(case, nblk + 1, what + ", packed, blk_cap = blocks + 1")  # grid = nblk + 1
    packed_raw(case, kv.n + 2, what + ", packed, blk_cap = entries + 2")  # grid = entries + 1
    slots(case, what + ", slots")
    framed_check(kv, seg, 4096, ref_blocks, ref_off)


@pytest.mark.parametrize("nblk", NBLK)
@pytest.mark.parametrize("mode", MODES)
def test_block_counts_on_the_group_edges(mode, nblk, emit_mode):
    emit_mode(mode)
    three_outputs(case_of(nblk), f"{nblk} blocks, mode {mode}")


@pytest.mark.parametrize("clamp", [64, 72])
@pytest.mark.parametrize("mode", MODES)
def test_clamped_grid_strides(mode, clamp, emit_mode):
    """200 blocks under 64 workgroups (one whole group, three or four strides each) and under 72 (a
    whole group and a partial one of 8, strides of 72)."""
    emit_mode(mode, clamp)
    three_outputs(case_of(200), f"200 blocks, grid clamped to {clamp}, mode {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_empty_and_one_entry_segments(mode, emit_mode):
    for clamp in (0, 72):
        emit_mode(mode, clamp)
        three_outputs(case_edge_segments(), f"empty + one-entry segment, clamp {clamp}, mode {mode}")


@pytest.mark.parametrize("clamp", [0, 64, 72])
@pytest.mark.parametrize("mode", MODES)
def test_capacity_one_byte_short_of_the_last_block(mode, clamp, emit_mode):
    """out_cap one byte short of the last block: LSMBLK_E_CAPACITY, every earlier block byte-exact,
    the bytes from the last block's start on keep their fill."""
    emit_mode(mode, clamp)
    kv, seg, ref_blocks, ref_off = case_of(200)
    total, last = int(ref_off[-1]), int(ref_off[-2])
    status, st, got, off = raw_encode(to_dev(kv), seg, total - 1, kv.n + 2, total)
    assert status == LSMBLK_E_CAPACITY
    assert st[0] == len(ref_off) - 1
    assert_bytes(got[:last], ref_blocks[:last], ref_off, "blocks before the last")
    assert (got[last:] == FILL).all(), "bytes past the last written block changed"
