"""The snapshot range-scan cases (lsm_scan_newest_cases.py) without a GPU: the closed form the device
test compares against equals a plain per-key maximum and a heap merge followed line by line on every
range, it equals the MVCC mode wherever no key lives in two sources and the NEWEST point read on every
point range, the rank and visibility argument of lsm_scan_rank_kernel<true> holds on every range, the
generators reach what they were built for, and the flag is declared in every layer."""
import bisect
import os
import re

import pytest

import lsm_get_cases as lc
import lsm_scan_cases as ls
import lsm_scan_newest_cases as ln
import scan_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,bs", ln.CASES)
def test_every_table_meets_the_precondition(name, bs):
    """(key ascending, ts descending), strictly: the order the mode's contract asks of every table."""
    for s in ln.case(name, bs).view.ssts:
        ents = [(k, -ts) for k, ts, _ in lc.flat(s)[0]]
        assert all(x < y for x, y in zip(ents, ents[1:]))


@pytest.mark.parametrize("name,bs", ln.CASES)
def test_the_three_routes_agree_on_every_range(name, bs):
    c = ln.case(name, bs)
    view, merged = ln.rows(name, bs, "view"), ln.rows(name, bs, "merged")
    assert len(view) == len(merged) == len(c) > 0
    for i, (lk, lo, uk, up, ts) in enumerate(c.ranges()):
        where = (i, lk, lo, uk, up, ts)
        r, m = view[i], merged[i]
        assert r["out"] == ln.plain_newest(c.view, lk, lo, uk, up, ts), where
        assert r["out"] == ln.line_by_line_newest(c.view, lk, lo, uk, up, ts), where
        assert m["out"] == ln.line_by_line_newest(c.view, lk, lo, uk, up, None), where
        assert sorted(m["out"]) == ln.every_version(c.view, lk, lo, uk, up), where
        order = [(k, -t) for k, t, _ in m["out"]]
        assert order == sorted(order), where
        for x in (r, m):
            assert x["merged"] == x["raw"] == len(m["out"]) and x["n"] == len(x["out"]), where
            assert x["status"] == (ln.OK if x["out"] else ln.EMPTY), where
        assert r["sources"] == m["sources"] == len(r["runs"])


@pytest.mark.parametrize("name,bs", ln.CASES)
def test_equals_the_mvcc_mode_where_no_key_lives_in_two_sources(name, bs):
    c = ln.case(name, bs)
    nonempty = several = 0
    for i, (lk, lo, uk, up, ts) in enumerate(c.ranges()):
        runs = ls.runs_of(c.view, lk, lo, uk, up, True)
        if runs is None or not ln.disjoint(runs):
            continue
        for mode, read_ts in (("view", ts), ("merged", None)):
            old = ls.closed(c.view, lk, lo, uk, up, True, read_ts)
            assert ln.rows(name, bs, mode)[i]["out"] == old["out"], (i, mode)
        nonempty += any(r for _, r in runs)
        several += sum(1 for _, r in runs if r) >= 2
    assert nonempty > 0
    if name in ls.VIEWS:  # (owners and versions share their keys between sources on purpose)
        assert several > 0


@pytest.mark.parametrize("name,bs", (("versions", 128), ("owners", 128)))
def test_point_ranges_equal_the_newest_point_read(name, bs):
    c = ln.case(name, bs)
    idx = ln.point_ranges(name, bs)
    assert len(idx) >= 40
    found = hidden = 0
    for i in idx:
        got = ln.rows(name, bs, "view")[i]["out"]
        best = lc.newest_plain(c.view, c.lower[i], c.read_ts[i])
        if best is not None and best[2]:
            assert got == [(c.lower[i], best[0], best[2])], i
            found += 1
        else:
            assert got == [], i
            hidden += best is not None
    assert found >= 10 and hidden >= 3


def kernel_model(runs, read_ts):
    """lsm_scan_rank_kernel<true>'s argument over one range's runs: per entry e of run r its place
    pos = i + sum(ub(r') for r' < r) + sum(lb(r') for r' > r) under the (key, ts descending) order, and
    hidden iff some run's last entry before e in merged order has e's key and a ts <= read_ts
    -> the slots, None where the reader's view keeps nothing."""
    order = [[(k, -ts) for k, ts, _ in run] for run in runs]
    slot = [None] * sum(len(r) for r in runs)
    for r, run in enumerate(runs):
        for i, e in enumerate(run):
            pos, keep = i, read_ts is None or (e[1] <= read_ts and bool(e[2]))
            for r2, other in enumerate(order):
                p = i if r2 == r else (bisect.bisect_right if r2 < r else bisect.bisect_left)(other, order[r][i])
                pos += p if r2 != r else 0
                if read_ts is not None and p > 0 and runs[r2][p - 1][0] == e[0] and runs[r2][p - 1][1] <= read_ts:
                    keep = False
            assert slot[pos] is None  # a bijection
            slot[pos] = (e, keep)
    return [e for e, keep in slot if keep]


@pytest.mark.parametrize("name,bs", ln.CASES)
def test_the_rank_and_visibility_argument_holds_on_every_range(name, bs):
    c = ln.case(name, bs)
    for i, ts in enumerate(c.read_ts):
        for mode, read_ts in (("view", ts), ("merged", None)):
            r = ln.rows(name, bs, mode)[i]
            assert kernel_model(r["runs"], read_ts) == r["out"], (i, mode)


def test_every_class_is_reached():
    ver = ln.classes("versions", 128)
    for k in ln.CLASSES:
        if k != "over_64_runs":
            assert ver[k] > 0, k
    own = ln.classes("owners", 128)
    for k in ("winner_not_highest_priority", "newest_differs_from_mvcc", "all_image_tie"):
        assert own[k] > 0, k
    for bs in (128, 256):
        assert ln.classes("levels", bs)["over_64_runs"] > 0
    for name, bs in ln.CASES:
        assert ln.classes(name, bs)["run_len_0"] > 0, (name, bs)


def test_cases_cover_the_bound_kinds_and_read_ts_values_and_stay_small():
    c = ln.case("versions", 128)
    assert {(a, b) for a, b in zip(c.lkind, c.ukind)} == {(a, b) for a in sc.KINDS for b in sc.KINDS}
    assert {0, ln.TS_MID, ln.TS_MAX} <= set(c.read_ts)
    assert sum(len(s.entries) for s in c.view.ssts) <= 400
    for name, bs in ln.CASES:
        exp, _, _ = ln.expected(name, bs, "view")
        assert int(exp["raw"].sum()) <= 20000, (name, bs)


def test_the_flag_is_declared_in_every_layer():
    import inspect

    from lsm_amd import _lib, sst
    header = open(os.path.join(ROOT, "include", "lsmblk.h")).read()
    assert re.search(r"#define\s+LSMBLK_LSM_SCAN_NEWEST\s+4u", header)
    assert _lib.LSMBLK_LSM_SCAN_NEWEST == _lib.LSMBLK_LSM_GET_NEWEST == ln.NEWEST == 4
    assert inspect.signature(sst.SstSet.lsm_scan).parameters["newest"].default is False
