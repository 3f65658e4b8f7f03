"""The inputs of tests/merge_newest_cases.py, checked on the CPU: the two routes to the
LSMBLK_MERGE_NEWEST order agree on every case, every generator reaches the path it was built for
(and fails that check against other constants), the order is MergeIterator's where no key lives in
two runs, and the reason for the mode stated as a test: a snapshot reader's rows survive a
compaction over the NEWEST order and not one over the run-priority order.
test_gpu_merge_newest.py runs the same inputs on the device."""
import dataclasses
import os
import re

import numpy as np
import pytest

import compact_cases as cc
import merge_newest_cases as mn
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def other(**kw):
    return dataclasses.replace(cc.C, **kw)


@pytest.fixture(scope="module")
def cases():
    return mn.merge_cases()


def test_the_mode_is_exported_and_defined_in_the_header():
    from lsm_amd import _lib
    assert _lib.LSMBLK_MERGE_NEWEST == 2 == mn.NEWEST
    header = open(os.path.join(ROOT, "include", "lsmblk.h")).read()
    assert re.search(r"^#define\s+LSMBLK_MERGE_NEWEST\s+2u\s*$", header, re.M)
    assert (_lib.LSMBLK_MERGE_RUNS, _lib.LSMBLK_MERGE_TWO_LEVEL) == (0, 1)


def test_the_two_routes_agree_on_every_case(cases):
    for name, case in cases.items():
        assert mn.runs_in_order(case), name
        a, b = mn.newest_order(case), mn.heap_order(case)
        assert a.tolist() == b.tolist(), name
        assert sorted(a.tolist()) == list(range(case.kv.n)), name   # every input entry, once
        ents = [case.kv.entry(int(i)) for i in a]
        assert all((x[0], -x[1]) <= (y[0], -y[1]) for x, y in zip(ents, ents[1:])), name
    for name, case, *_ in mn.rules_cases():
        assert mn.newest_order(case).tolist() == mn.heap_order(case).tolist(), name


def test_the_small_cases_hold_what_they_were_built_for(cases):
    hot = mn.check_interleaved(cases["interleaved"])
    mn.check_u64_edges(cases["u64_edges"])
    nmulti = mn.check_key_ties(cases["key_ties"])
    eq = cases["equal_ts"]
    order = [eq.kv.entry(int(i)) for i in mn.newest_order(eq)]
    assert [v for k, ts, v in order if k == b"e-equal" and ts == 4] == [b"e0.4", b"e1.4", b"e2.4"]   # run order decides
    assert [v for k, ts, v in order if k == b"f-equal"][:3] == [b"f0", b"", b"f2"]
    many = cases["many_runs"]
    assert len(many.rs) - 1 == 64 and set(np.diff(many.rs.astype(np.int64)).tolist()) == {1, 2, 3}
    assert len(mn.multi_run_keys(many)) >= 10
    er = np.diff(cases["empty_runs"].rs.astype(np.int64))
    assert er[0] == 0 and er[-1] == 0 and (er[2:4] == 0).all() and er[1] and er[4]
    one = cases["single_run"]
    assert len(one.rs) == 2 and mn.newest_order(one).tolist() == list(range(one.kv.n))
    assert cases["no_entries"].kv.n == 0 and mn.newest_order(cases["no_entries"]).tolist() == []
    print(f"interleaved: (run, ts) of the hot key {hot}; key ties: {nmulti} keys in two runs")


def test_tile_limits_reach_all_three_tile_paths():
    c = cc.C
    kernels = [mn.check_tile_limit(mn.tile_limit(X)) for X in mn.tile_limit_sizes()]
    assert tuple(kernels) == mn.TILE_KERNELS and {"tile", "big", "global"} == set(kernels)
    # built for other constants the probes leave the limits, and the check notices
    for c2 in (other(kMTE=c.kMTE + 128), other(kBigTE=c.kBigTE - 500)):
        with pytest.raises(AssertionError):
            for X in mn.tile_limit_sizes():
                mn.check_tile_limit(mn.tile_limit(X), c2)
        assert tuple(mn.check_tile_limit(mn.tile_limit(X, c2), c2) for X in mn.tile_limit_sizes(c2)) == mn.TILE_KERNELS
    with pytest.raises(AssertionError):   # other candidate positions: other tiles
        mn.check_tile_limit(mn.tile_limit(c.kMTE), other(kMS=c.kMS * 4))
    print("tile-limits:", dict(zip(mn.tile_limit_sizes(), kernels)))


def test_candidate_edges_put_the_shared_key_on_candidates(cases):
    c = cc.C
    big = mn.check_cand_edges(cases["cand_edges"])
    assert big >= c.kMS + 4   # the shared key's tile: all its versions from the four runs
    with pytest.raises(AssertionError):
        mn.check_cand_edges(cases["cand_edges"], other(kMS=c.kMS * 2))
    c2 = other(kMS=c.kMS // 2)
    mn.check_cand_edges(mn.cand_edges(c2), c2)


def test_rules_cases_reach_every_rule_class():
    seen = mn.check_rules_cases(mn.rules_cases())
    print("rules:", sorted(seen))


def test_rotation_holds_cuts_back_inside_versions_from_several_runs(cases):
    held, nsst = mn.check_rotation(cases["rotation"])
    print(f"rotation: {nsst} SSTs, {held} cuts held back over versions from several runs")


def test_disjoint_runs_give_the_merge_iterators_order(cases):
    """Where no key lives in two runs the modes coincide."""
    case = cases["disjoint"]
    assert not mn.multi_run_keys(case) and len(case.rs) - 1 == 4 and case.kv.n > 300
    assert mn.newest_order(case).tolist() == O.merge_runs(case.kv, case.rs).tolist()
    for name in ("single_run", "no_entries"):
        assert mn.newest_order(cases[name]).tolist() == O.merge_runs(cases[name].kv, cases[name].rs).tolist()
    assert mn.newest_order(cases["interleaved"]).tolist() != O.merge_runs(cases["interleaved"].kv, cases["interleaved"].rs).tolist()


@pytest.mark.parametrize("name", ["interleaved", "equal_ts", "key_ties", "many_runs"])
def test_snapshot_rows_survive_a_newest_compaction_and_not_a_runs_one(cases, name):
    """A snapshot reader's rows -- per key the newest version at or below T over all input entries,
    a tombstone hides -- are the same after compact_generate_sst over the NEWEST order for every
    T >= watermark, with and without bottom_level (no prefix filter); over the run-priority order
    they differ for some T >= watermark."""
    case = cases[name]
    ents = case.kv.entries()
    tss = sorted({ts for _, ts, _ in ents})
    newest, runs = mn.newest_order(case), O.merge_runs(case.kv, case.rs)
    before = [ents[int(i)] for i in newest]   # (equal ts: the lower run first, as the snapshot read takes them)
    differs = 0
    for wm in [0] + tss:
        reads = [T for T in tss + [tss[-1] + 1, mn.U64] if T >= wm]
        for bottom in (False, True):
            kept = O.compact(case.kv, newest, wm, bottom, (), 4096, 1 << 20, kept_only=True)["kept"]
            after = [before[int(j)] for j in kept]
            for T in reads:
                assert mn.snapshot_rows(after, T) == mn.snapshot_rows(before, T), (wm, bottom, T)
            kept = O.compact(case.kv, runs, wm, bottom, (), 4096, 1 << 20, kept_only=True)["kept"]
            after = [ents[int(runs[int(j)])] for j in kept]
            differs += sum(mn.snapshot_rows(after, T) != mn.snapshot_rows(before, T) for T in reads)
    assert differs > 0
    if name == "interleaved":   # the issue's example: m-two at T = 6 reads run 1's ts 5, gone after a RUNS compaction
        after = [ents[int(runs[int(j)])] for j in O.compact(case.kv, runs, 0, False, (), 4096, 1 << 20, kept_only=True)["kept"]]
        assert (b"m-two", 5, b"r1@5") in mn.snapshot_rows(before, 6) and \
            not any(k == b"m-two" for k, _, _ in mn.snapshot_rows(after, 6))
