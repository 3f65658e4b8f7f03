"""The LSM range-scan cases (lsm_scan_cases.py) without a GPU: the closed form the device test
compares against equals scan_with_ts's iterators followed line by line on every range, the one
deliberate difference from the reference (LsmIterator::new's untested first position) is exactly
that, the generators reach what they were built for, and the call is declared in every layer."""
import os
import re

import pytest

import lsm_scan_cases as ls
import scan_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", ls.MODES)
@pytest.mark.parametrize("name,bs", ls.CASES)
def test_closed_form_equals_line_by_line_on_every_range(name, bs, mode):
    c = ls.case(name, bs)
    mvcc, filt = ls.mode_args(mode)
    rws = ls.rows(name, bs, mode)
    assert len(rws) == len(c) > 0
    for i, (lk, lo, uk, up, ts) in enumerate(c.ranges()):
        want = ls.line_by_line(c.view, lk, lo, uk, up, mvcc, ts if filt else None)
        assert rws[i]["out"] == want, (i, lk, lo, uk, up, ts)
        assert rws[i]["n"] == len(want) and rws[i]["status"] == (ls.OK if want else ls.EMPTY)
        assert rws[i]["merged"] <= rws[i]["raw"] and rws[i]["n"] <= rws[i]["merged"]
        if not filt:
            assert rws[i]["n"] == rws[i]["merged"]


@pytest.mark.parametrize("mvcc", (False, True))
def test_the_reference_iterator_differs_only_by_a_leading_entry_beyond_the_bound(mvcc):
    """scan_cases.LsmIterator as written does not test the end bound on its first position: its
    output is the closed form's, or the closed form is empty and it yields the one entry the merged
    iterator stood on, which lies beyond the bound."""
    quirk = 0
    for name, bs in ls.CASES:
        c = ls.case(name, bs)
        rws = ls.rows(name, bs, "mvcc" if mvcc else "default")
        for i, (lk, lo, uk, up, ts) in enumerate(c.ranges()):
            got = ls.line_by_line(c.view, lk, lo, uk, up, mvcc, ts, iterator=sc.LsmIterator)
            if got != rws[i]["out"]:
                assert rws[i]["out"] == [] and len(got) == 1 and not ls.within(got[0][0], uk, up), (name, bs, i)
                quirk += 1
    assert quirk > 0


def test_every_class_is_reached():
    tot = dict.fromkeys(ls.CLASSES, 0)
    for name, bs in ls.CASES:
        for k, x in ls.classes(name, bs).items():
            tot[k] += x
    for k in ls.CLASSES:
        assert tot[k] > 0, k
    own = ls.classes("owners", 128)
    for k in ("key_in_3_sources", "owner_blind_later_sees", "owner_tombstone", "all_image_tie", "merge_nonempty_view_empty") + \
            tuple("run_len_%d" % n for n in ls.RUN_LENGTHS):
        assert own[k] > 0, k
    for bs in (128, 256):
        lv = ls.classes("levels", bs)
        assert lv["level_span_ge_65"] > 0 and lv["over_64_runs"] > 0
        assert ls.classes("ties", bs)["all_image_tie"] > 0
    for name, bs in ls.CASES:
        n = ls.classes(name, bs)
        for k in ("begin_mid_versions", "no_source", "merge_nonempty_view_empty", "lower_gt_upper", "run_len_0"):
            assert n[k] > 0, (name, bs, k)
    assert sum(ls.classes(n, b)["excl_skip_across_block"] for n, b in ls.CASES) > 0


def test_cases_cover_the_bound_kinds_and_read_ts_values_and_stay_small():
    for name, bs in ls.CASES:
        c = ls.case(name, bs)
        assert {(a, b) for a, b in zip(c.lkind, c.ukind)} == {(a, b) for a in sc.KINDS for b in sc.KINDS}
        assert {0, ls.TS_MID, ls.TS_MAX} <= set(c.read_ts)
        exp, _, _ = ls.expected(name, bs, "default")
        assert int(exp["raw"].sum()) <= 8000, (name, bs)


def test_the_call_is_declared_in_every_layer():
    from lsm_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsmblk.h")).read()
    assert re.search(r"^int lsmblk_lsm_scan_batch\(", header, re.M)
    assert "#define LSMBLK_LSM_SCAN_STATS_WORDS 8" in header and "} lsmblk_lsm_scan_result;" in header
    assert "lsmblk_lsm_scan_batch" in [n for n, _, _ in _lib.SIGNATURES]
    assert "pub fn lsmblk_lsm_scan_batch(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    import ctypes
    assert ctypes.sizeof(_lib.LsmScanResultC) == 32
