"""GPU parity on the edge between walk_segment's anchored pass and its carried-window loop: blocks of
63, 64 and 65 entries, a 64-entry block that ends with its segment, anchored windows that wrap the
ring, a long block followed by short ones, out-of-order pairs on lanes 1 and 63 of an anchored window,
segments of 1 and 65 entries -- with either helper (plan_produce, plan_produce_pipe) through the
packed encode, the unfused and the fused slot encode and the framed encode.

The inputs and their coverage conditions are tests/walk_anchored_cases.py's (checked on the CPU by
test_walk_anchored_cases.py).  Expected offsets and bytes come from the oracle only.
"""
import functools

import pytest

import walk_anchored_cases as wa
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch
from lsm_amd._lib import LSMBLK_DEBUG_PLAN_PIPE, lib
from oracle import oracle as O
from test_gpu_parity import framed_check, slot_check, to_dev
from test_gpu_paths import packed_check

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 1], ids=["plan_produce", "plan_produce_pipe"])
def helper(request):
    ctx = batch._ctx(0)
    assert lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_PLAN_PIPE, request.param) == 0
    yield request.param
    assert lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_PLAN_PIPE, 0) == 0


@functools.lru_cache(maxsize=None)
def edges():
    """(case, oracle blocks, oracle offsets), the restatement's table checked against the oracle's."""
    case = wa.edges()
    rc, ref_blocks, ref_off = O.encode_segments(*case)
    assert rc == 0
    for a in (ref_blocks, ref_off):
        a.setflags(write=False)
    W = wa.AnchoredWalk(*case)
    wa.check_table(W, ref_blocks, ref_off)
    wa.check_edges(W, case[1])
    print(wa.walk_line("edges", W))
    return case, ref_blocks, ref_off


def test_packed(helper):
    """The block table (offsets) and the bytes of the packed encode."""
    (kv, seg, bs), ref_blocks, ref_off = edges()
    packed_check(to_dev(kv), seg, bs, ref_blocks, ref_off, f"edges, helper {helper}")


def test_slots_unfused_and_fused(helper):
    """plan_walk_kernel and the fused launch share walk_segment."""
    (kv, seg, bs), ref_blocks, ref_off = edges()
    slot_check(kv, seg, bs, ref_blocks, ref_off)


def test_framed(helper):
    (kv, seg, bs), ref_blocks, ref_off = edges()
    framed_check(kv, seg, bs, ref_blocks, ref_off)
