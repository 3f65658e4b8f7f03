"""CPU tests of lsm_get_cases.py: the closed form of lsmblk_lsm_get_batch equals the line-by-line
get_with_ts composition on every query of every case, NEWEST equals a plain maximum, the views are
valid, the cases reach the input classes they were built for, and the ABI bookkeeping is in place."""
import ctypes
import os
import re

import pytest

import lsm_get_cases as lc
from lsm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,bs", lc.CASES)
@pytest.mark.parametrize("mode", ("default", "mvcc"))
def test_closed_form_equals_line_by_line(name, bs, mode):
    v = lc.case(name, bs)
    for r, key, ts in zip(lc.rows(name, bs, mode), v.keys, v.read_ts):
        got = lc.line_by_line(v, key, ts, mode == "mvcc")
        want = (r["value"], r["ts"]) if r["status"] == lc.FOUND else None
        assert got == want, (key, ts, r, got)


@pytest.mark.parametrize("name,bs", lc.CASES)
def test_newest_equals_plain_maximum(name, bs):
    v = lc.case(name, bs)
    for r, key, ts in zip(lc.rows(name, bs, "newest"), v.keys, v.read_ts):
        best = lc.newest_plain(v, key, ts)
        if best is None:
            assert r["status"] == lc.ABSENT and r["src"] == lc.NONE and r["hit_blk"] == lc.NONE, (key, ts, r)
        else:
            assert (r["ts"], r["src"]) == best[:2] and r["status"] == (lc.FOUND if best[2] else lc.TOMBSTONE), (key, ts, r)
            assert r["value"] == (best[2] or None)


@pytest.mark.parametrize("name,bs", lc.CASES)
def test_views_are_valid(name, bs):
    """check_sst_valid holds, so a level never has two tables passing key_within."""
    v = lc.case(name, bs)
    for lv in v.levels:
        for x, y in zip(lv, lv[1:]):
            assert lc.last_key(v.ssts[x]) < lc.first_key(v.ssts[y])
        for key in v.keys:
            assert sum(lc.first_key(v.ssts[t]) <= key <= lc.last_key(v.ssts[t]) for t in lv) <= 1
    assert all(len(s.entries) >= 2 for s in v.ssts)


def test_rows_have_the_record_shape():
    for name, bs in lc.CASES:
        for mode in lc.MODES:
            for r in lc.rows(name, bs, mode):
                hit = r["status"] in (lc.FOUND, lc.TOMBSTONE)
                assert (r["hit_blk"] != lc.NONE) == hit and (r["val_pos"] is not None) == hit
                assert (r["src"] == lc.NONE) == (r["sst"] == lc.NONE)
                assert r["status"] in (lc.ABSENT, lc.FOUND, lc.TOMBSTONE)
                if mode == "newest":
                    assert (r["src"] != lc.NONE) == hit


REACHED = {
    "mixed": ("decider_src0", "decider_later_l0", "decider_level", "earlier_false_positive", "earlier_bloom_out",
              "earlier_range_out", "decider_blind_later_sees", "default_mvcc_differ", "mvcc_newest_differ", "tombstone",
              "level_gap", "level_below", "level_above"),
    "levels": ("decider_level", "level_gap", "level_below", "level_above", "level_over_64"),
    "ties": ("image_tie", "decider_level", "level_gap"),
    "threshold": ("big_block_later_source", "decider_later_l0", "decider_level"),
}


@pytest.mark.parametrize("name,bs", [c for c in lc.CASES if c[0] in REACHED])
def test_cases_reach_their_classes(name, bs):
    n = lc.classes(name, bs)
    print(name, bs, n)
    for c in REACHED[name]:
        assert n[c] >= (20 if name == "mixed" else 1), (c, n)


def test_levels_case_has_the_sizes_around_the_probe_step():
    v = lc.case("levels", 128)
    assert [len(lv) for lv in v.levels] == [1, 3, 0, 64, 65, 70]
    assert all(2 <= len(v.ssts[t].entries) <= 4 for lv in v.levels for t in lv)


def test_ties_case_has_the_shared_prefixes():
    v = lc.case("ties", 128)
    a, b = ([lc.first_key(v.ssts[t]) for t in lv] for lv in v.levels)
    assert len(a) >= 5 and len(set(a)) == len(a) and all(k.startswith(lc.TIE_PREFIX) for k in a)
    assert len(set(b)) == len(b) and all(k.startswith(lc.TIE_PREFIX[:14]) for k in b)
    assert {lc.TIE_PREFIX, lc.TIE_PREFIX[:16], lc.TIE_PREFIX[:16] + b"\x00"} <= set(v.keys)


def test_edges_views():
    assert lc.case("edges_levels", 128).l0 == [] and lc.case("edges_levels", 128).levels
    assert lc.case("edges_l0", 256).levels == [] and lc.case("edges_l0", 256).l0
    many = lc.case("edges_72_sources", 128)
    assert many.nsrc > 64 and len(many.l0) > 64 and {r["src"] for r in lc.rows("edges_72_sources", 128, "default")} & {70, 71}
    assert len(lc.case("edges_one64", 128).levels[0]) == 64
    e = lc.case("edges_empty", 128)
    assert e.nsrc == 0
    for mode in lc.MODES:
        assert all(r["status"] == lc.ABSENT and r["src"] == lc.NONE and r["seeks"] == 0 for r in lc.rows("edges_empty", 128, mode))


def test_abi_declares_binds_and_documents_the_call():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsmblk.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+lsmblk_lsm_get_batch\s*\(", header)
    assert "lsmblk_lsm_get_batch" in {n for n, _, _ in _lib.SIGNATURES}
    assert "pub fn lsmblk_lsm_get_batch(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"#define\s+LSMBLK_LSM_GET_NEWEST\s+4u", header) and _lib.LSMBLK_LSM_GET_NEWEST == 4


def test_result_record_is_48_bytes():
    assert ctypes.sizeof(_lib.LsmGetResultC) == 48
    assert _lib.LsmGetResultC.seeks.offset == 40 and _lib.LsmGetResultC.val_pos.offset == 32
    assert _lib.LsmGetResultC.vlen.offset == _lib.GetResultC.vlen.offset  # the value gather reads either record
