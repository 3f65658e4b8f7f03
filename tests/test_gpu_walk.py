"""GPU parity on the encode plan walk: every route of the helper's LCP and order decision at every
alignment of the key arena, and walk_segment's window geometry, ring wrap, direct mode, fused
multi-segment walkers and 64-bit arithmetic, through plan_produce and plan_produce_pipe, hosted by
plan_walk_kernel and by the fused launch.

The inputs and the coverage conditions are tests/walk_cases.py's (checked on the CPU by
test_walk_cases.py); the conditions that depend on the device are asserted again here, for the key
arena's real address and the device's CU count.  Expected offsets and bytes come from the oracle only.
"""
import pytest
import torch

import walk_cases as wc
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch
from lsm_amd._lib import LSMBLK_DEBUG_PLAN_PIPE, lib
from oracle import oracle as O
from test_gpu_parity import framed_check, slot_check, to_dev
from test_gpu_paths import decode_check, packed_check, rehome

pytestmark = pytest.mark.gpu


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def both_helpers(d, seg, bs, ref_blocks, ref_off, what):
    """The packed encode through plan_produce, then through plan_produce_pipe."""
    packed_check(d, seg, bs, ref_blocks, ref_off, what)
    ctx = batch._ctx(0)
    assert lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_PLAN_PIPE, 1) == 0
    try:
        packed_check(d, seg, bs, ref_blocks, ref_off, what + ", pipelined helper")
    finally:
        lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_PLAN_PIPE, 0)


def run_case(case, what, slots=True, framed=True, decode=True):
    """Packed encode with either helper, slot encode unfused and fused, framed encode, decode of the
    oracle's blocks -> (device stream, oracle blocks, oracle offsets)."""
    kv, seg, bs = case
    rc, ref_blocks, ref_off = O.encode_segments(kv, seg, bs)
    assert rc == 0
    d = to_dev(kv)
    both_helpers(d, seg, bs, ref_blocks, ref_off, what)
    if slots:
        slot_check(kv, seg, bs, ref_blocks, ref_off)
    if framed:
        framed_check(kv, seg, bs, ref_blocks, ref_off)
    if decode:
        rc, ref_kv = O.decode_blocks(ref_blocks, ref_off)
        if rc == 0:
            decode_check(ref_blocks, ref_off, ref_kv, what=what)
    return d, ref_blocks, ref_off


def rehomed_helpers(case, what, seen):
    """Either helper with the key arena at every address mod 16; the pairs' (route, sorted, z & 3)
    under the arena's real address go into seen[glead]."""
    kv, seg, bs = case
    d, ref_blocks, ref_off = run_case(case, what)
    for shift in range(16):
        d = to_dev(kv)
        d.keys = rehome(d.keys, shift)
        both_helpers(d, seg, bs, ref_blocks, ref_off, f"{what}, key arena at {shift} mod 16")
        P = wc.classify_pairs(kv, seg, d.keys.data_ptr())
        assert P.glead == shift
        seen.setdefault(shift, set()).update(P.seen())
    return P


def test_pair_probes_every_route_and_alignment():
    """[F, A, B] per segment: A and B first differing at z in 0..19 and 31..33 by (7F, 80), (00, 01),
    (FE, FF) in either order with the later bytes ordered the other way, prefix pairs of 1..20 bytes,
    shortcut-defeating triples -- a pair wrongly judged sorted changes a prefix in the output."""
    case = wc.pair_probes()
    seen = {}
    P = rehomed_helpers(case, "pair_probes", seen)
    want = {(r, s, q) for r in ("select", "dword") for s in (False, True) for q in range(4)}
    for glead in range(16):
        assert want <= seen[glead], f"glead {glead}: missing {sorted(want - seen[glead])}"
    print(wc.pairs_line("pair_probes", P))


def test_tail_probes_every_alignment():
    """Streams whose last keys are 1 to 15 bytes long: the pairs within 16 bytes of the arena's end
    (key_diff through alignbyte loads), sorted, unsorted and prefixes."""
    seen = {}
    for i, case in enumerate(wc.tail_probes()):
        P = rehomed_helpers(case, f"tail_probes[{i}]", seen)
    want = {("tail", s, q) for s in (False, True) for q in range(4)}
    for glead in range(16):
        assert want <= seen[glead], f"glead {glead}: missing {sorted(want - seen[glead])}"
    print(wc.pairs_line("tail_probes (last stream)", P))


def test_window_geometry():
    """Blocks starting and ending on lanes 0, 1 and 63, many ends in one window, blocks open over three
    windows from the outer path and from the inner loop, the reject rule at block_size and
    block_size + 1 on the outer path and in the inner loop, segments on the edges of kPipeE, kChunk
    and kRing."""
    case = wc.geometry()
    _, ref_blocks, ref_off = run_case(case, "geometry")
    W = wc.Walk(*case)
    wc.check_table(W, ref_blocks, ref_off)
    wc.check_geometry(W, case[1])
    print(wc.walk_line("geometry", W))


def test_direct_mode_rewraps_the_ring():
    """Segments longer than 2 kRing with an out-of-order pair every few blocks: direct mode re-anchors
    the window grid, windows hold ring slots kRing - 1 and 0."""
    case = wc.direct_rewrap()
    _, ref_blocks, ref_off = run_case(case, "direct_rewrap")
    P = wc.classify_pairs(case[0], case[1])
    W = wc.Walk(*case, pairs=P)
    wc.check_table(W, ref_blocks, ref_off)
    wc.check_direct_rewrap(W, case[1], P)
    print(wc.walk_line("direct_rewrap", W))


def test_fused_walkers_take_several_segments():
    """More than 2 nwalk segments: every fused walker walks three segments on one ring based at its
    first, and later segments' windows straddle the ring wrap."""
    cus = cu_count()
    case = wc.fused_multi(cus)
    nwalk, spw = wc.fused_shape(cus, len(case[1]) - 1)
    assert spw >= 2
    _, ref_blocks, ref_off = run_case(case, "fused_multi")
    W = wc.Walk(*case, ring_base=wc.fused_ring_base(case[1], spw))
    wc.check_table(W, ref_blocks, ref_off)
    assert wc.check_fused_multi(W, case[1], cus) == (nwalk, spw)
    print(f"{cus} CUs, {nwalk} walkers x {spw} segments; " + wc.walk_line("fused_multi", W))


def test_wide_block_sizes():
    """block_size 2^30 - 1, 2^30, 2^31, 2^32 - 1: either side of the u32 path."""
    for case in wc.wide():
        _, ref_blocks, ref_off = run_case(case, f"wide {case[2]}", slots=False, framed=False, decode=False)
        W = wc.Walk(*case)
        wc.check_table(W, ref_blocks, ref_off)
        wc.check_wide(W, case[2])
        print(wc.walk_line(f"wide {case[2]}", W))


def test_huge_entries():
    """Entries of r = 2^25 - 17 and 2^25 - 16 first in a segment, met by the inner loop, and inside a
    carried block; one accepted into a block at block_size 2^25 + 4096.  (The blocks wrap the u16
    fields: offsets and bytes only.)"""
    for which, case in enumerate(wc.huge()):
        kv, seg, bs = case
        _, ref_blocks, ref_off = run_case(case, f"huge {which}", slots=False, framed=False, decode=False)
        if which == 0:
            slot_check(kv, seg, bs, ref_blocks, ref_off)
        W = wc.Walk(*case)
        wc.check_table(W, ref_blocks, ref_off)
        wc.check_huge(W, which)
        print(wc.walk_line(f"huge {which}", W))
        del kv, ref_blocks
        torch.cuda.empty_cache()
