"""The anchored plan walk's edge inputs (tests/walk_anchored_cases.py), checked on the CPU: the
lane-level restatement of walk_segment -- the anchored pass in front of the carried-window loop -- must
find the oracle's block table on them and on walk_cases' streams, and must report the routes the
inputs were built for.  test_gpu_walk_anchored.py runs the same inputs on the device."""
import numpy as np
import pytest

import path_cases as pc
import walk_anchored_cases as wa
import walk_cases as wc
from oracle import oracle as O


def walked(case, decodes=True, ring_base=None):
    kv, seg, bs = case
    rc, blocks, off = O.encode_segments(kv, seg, bs)
    assert rc == 0
    if decodes:
        rc, back = O.decode_blocks(blocks, off)
        assert rc == 0 and pc.kv_equal(back, kv), "generator: the oracle does not read its own blocks back"
    W = wa.AnchoredWalk(*case, ring_base=ring_base)
    wa.check_table(W, blocks, off)
    return W


def test_edges():
    case = wa.edges()
    W = walked(case)
    wa.check_edges(W, case[1])
    print(wa.walk_line("edges", W))


def test_edges_on_a_shared_ring():
    """The same stream on one ring based at entry 0 (a fused walker's later segments): the same table."""
    case = wa.edges()
    W = walked(case, ring_base=np.zeros(len(case[1]) - 1, np.int64))
    assert any(b.straddle for b in W.blocks)


@pytest.mark.parametrize("name", ["geometry", "direct_rewrap", "pair_probes"])
def test_walk_cases_streams(name):
    """walk_cases' geometry, direct-mode and pair-probe streams through the anchored restatement."""
    case = getattr(wc, name)()
    W = walked(case)
    assert any(b.route == "anchored" for b in W.blocks)
    if name != "geometry":
        assert any(b.route == "direct" for b in W.blocks)
    print(wa.walk_line(name, W))


def test_wide_and_huge():
    """Block sizes >= 2^30 and entries of r >= 2^25 - 16 never take the anchored pass."""
    for case in wc.wide():
        W = walked(case, decodes=False)
        assert all(b.route == "wide" for b in W.blocks) == (case[2] >= wc.kNarrowBs)
    W = walked(wc.huge()[0], decodes=False)
    big = [b for b in W.blocks if W.rec[b.first] >= wc.kHugeRec]
    assert big and all(b.route in ("wide", "inner") for b in big)
