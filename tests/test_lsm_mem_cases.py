"""CPU tests of lsm_mem_cases.py: for views with memtable runs the closed forms of
lsmblk_lsm_get_batch / lsmblk_lsm_scan_batch equal the line-by-line get_with_ts / scan_with_ts
compositions on every query of every case and mode, with no run they are the existing closed forms,
the generators reach what they were built for, and the ABI bookkeeping is in place."""
import ctypes
import os
import re

import pytest

import lsm_get_cases as lc
import lsm_mem_cases as mc
import lsm_scan_cases as ls
import lsm_scan_newest_cases as lsn
from lsm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,bs", mc.CASES)
@pytest.mark.parametrize("mode", ("default", "mvcc"))
def test_get_closed_form_equals_line_by_line(name, bs, mode):
    c = mc.case(name, bs)
    for r, key, ts in zip(mc.get_rows(name, bs, mode), c.keys, c.read_ts):
        got = mc.get_line_by_line(c, key, ts, mode == "mvcc")
        want = (r["value"], r["ts"]) if r["status"] == mc.FOUND else None
        assert got == want, (key, ts, r, got)


@pytest.mark.parametrize("name,bs", mc.CASES)
def test_get_newest_equals_plain_maximum(name, bs):
    c = mc.case(name, bs)
    for r, key, ts in zip(mc.get_rows(name, bs, "newest"), c.keys, c.read_ts):
        best = mc.get_newest_plain(c, key, ts)
        if best is None:
            assert r["status"] == mc.ABSENT and r["src"] == mc.NONE and r["hit_ent"] == mc.NONE, (key, ts, r)
        else:
            assert (r["ts"], r["src"]) == best[:2] and r["status"] == (mc.FOUND if best[2] else mc.TOMBSTONE), (key, ts, r)
            assert r["value"] == (best[2] or None)


@pytest.mark.parametrize("name,bs", mc.CASES)
@pytest.mark.parametrize("mode", mc.SCAN_MODES)
def test_scan_closed_form_equals_line_by_line(name, bs, mode):
    c = mc.case(name, bs)
    for r, (lk, lo, uk, up, ts) in zip(mc.scan_rows(name, bs, mode), c.scan.ranges()):
        assert mc.scan_line_by_line(c, lk, lo, uk, up, mode, ts) == r["out"], (lk, lo, uk, up, ts)
        assert r["raw"] == sum(len(x) for x in r["runs"]) and r["sources"] == len(r["runs"])
        if mode.startswith("newest"):
            assert r["merged"] == r["raw"]


@pytest.mark.parametrize("name,bs", (("mixed3", 128), ("many67", 128)))
def test_without_runs_the_closed_forms_are_the_existing_ones(name, bs):
    c = mc.without_runs(mc.case(name, bs))
    for mode in mc.GET_MODES:
        for key, ts in list(zip(c.keys, c.read_ts))[::3]:
            assert mc.closed_get(c, key, ts, mode) == lc.closed(c.view, key, ts, mode)
    for lk, lo, uk, up, ts in c.scan.ranges():
        for mode, mvcc, rts in (("default", False, ts), ("mvcc", True, ts), ("merged", False, None)):
            assert mc.closed_scan(c, lk, lo, uk, up, mode, ts) == ls.closed(c.view, lk, lo, uk, up, mvcc, rts)
        assert mc.closed_scan(c, lk, lo, uk, up, "newest", ts) == lsn.closed_newest(c.view, lk, lo, uk, up, ts)
        assert mc.closed_scan(c, lk, lo, uk, up, "newest_merged", ts) == lsn.closed_newest(c.view, lk, lo, uk, up, None)


def test_rows_have_the_record_shape():
    for name, bs in mc.CASES:
        c = mc.case(name, bs)
        for mode in mc.GET_MODES:
            for r in mc.get_rows(name, bs, mode):
                hit = r["status"] in (mc.FOUND, mc.TOMBSTONE)
                mem = r["src"] != mc.NONE and r["src"] < c.nmem
                assert (r["hit_ent"] != mc.NONE) == hit and (r["val_pos"] is not None) == hit
                assert (r["hit_blk"] != mc.NONE) == (hit and not mem)
                assert (r["sst"] == mc.NONE) == (mem or r["src"] == mc.NONE)
                assert r["seeks"] >= (r["src"] + 1 if mem else c.nmem) and (not mem or mode == "newest" or r["bloom_out"] == 0)
                if mem and hit:
                    assert c.start[r["src"]] <= r["hit_ent"] < c.start[r["src"] + 1]


def test_runs_obey_the_precondition():
    for name, bs in mc.CASES:
        for run in mc.case(name, bs).runs:
            assert run == sorted(run, key=lambda e: (e[0], -e[1]))
            assert all(1 <= len(k) <= 65535 and len(v) <= 65535 for k, _, v in run)
            assert len({(k, ts) for k, ts, _ in run}) == len(run)


def test_the_cases_cover_the_run_counts_and_lengths():
    nmem = {mc.case(n, bs).nmem for n, bs in mc.CASES}
    assert {1, 2, 3, 64} <= nmem
    lengths = {len(r) for n, bs in mc.CASES for r in mc.case(n, bs).runs}
    assert set(mc.RUN_LENGTHS) <= lengths
    assert all(len(r) == 0 for r in mc.case("allempty", 128).runs) and mc.case("allempty", 128).nmem == 3
    none = mc.case("nosst", 0)
    assert none.view.ssts == [] and none.view.nsrc == 0 and none.view.file_off == [0] and none.view.files == b""
    many = mc.case("many67", 128)
    assert many.nmem == 3 and len(many.view.l0) == 70 and many.nmem + many.view.nsrc > 64


GET_REACHED = {
    "mixed3": ("mem_mutable_immutable_two_tables", "mem_blind_table_sees", "mem_tombstone_over_table_value", "equal_ts_mem_wins",
               "three_versions_read_between", "below_first_key", "above_last_key", "prefix_of_landing", "extends_predecessor",
               "decider_mutable", "decider_immutable", "decider_table_after_runs", "newest_table_beats_run"),
    "ties2": ("image_tie", "decider_mutable", "decider_immutable", "decider_table_after_runs"),
    "many67": ("table_src_ge_64", "decider_immutable", "decider_table_after_runs"),
    "nmem64": ("table_src_ge_64", "decider_immutable", "below_first_key", "above_last_key"),
    "one": ("decider_mutable", "decider_table_after_runs", "mem_blind_table_sees"),
    "allempty": ("decider_table_after_runs",),
    "nosst": ("decider_mutable", "decider_immutable", "three_versions_read_between", "prefix_of_landing", "extends_predecessor"),
}
SCAN_REACHED = {
    "mixed3": mc.SCAN_CLASSES[:7] + mc.SCAN_CLASSES[8:],
    "ties2": mc.SCAN_CLASSES[:7] + ("mem_and_table_runs", "mem_owner_hides_table"),
    "many67": ("over_64_runs", "mem_and_table_runs", "slice_whole_run"),
    "nmem64": ("over_64_runs", "key_in_two_mem_runs", "slice_empty", "slice_one", "overlap_fails_below", "overlap_fails_above"),
    "one": mc.SCAN_CLASSES[:7],
    "nosst": mc.SCAN_CLASSES[:7] + ("key_in_two_mem_runs",) + mc.SCAN_CLASSES[11:],
}


@pytest.mark.parametrize("name,bs", mc.CASES)
def test_cases_reach_their_classes(name, bs):
    g, s = mc.get_classes(name, bs), mc.scan_classes(name, bs)
    print(name, g, s)
    for k in GET_REACHED[name]:
        assert g[k] >= 1, (k, g)
    for k in SCAN_REACHED.get(name, ()):
        assert s[k] >= 1, (k, s)
    if name == "ties2":
        assert g["image_tie"] >= 100
    if name == "allempty":  # nothing of a run is reached, every answer is a table's with its ordinal shifted by three
        assert all(v == 0 for k, v in g.items() if k != "decider_table_after_runs")
        assert all(r["src"] == mc.NONE or r["src"] >= 3 for r in mc.get_rows(name, bs, "mvcc"))


def test_view_struct_is_56_bytes_with_the_runs_last():
    V = _lib.LsmViewC
    assert ctypes.sizeof(V) == 56
    assert [f[0] for f in V._fields_] == ["l0", "nl0", "nlevel", "level_sst", "level_start", "mem", "mem_start", "nmem"]
    assert (V.level_start.offset, V.mem.offset, V.mem_start.offset, V.nmem.offset) == (24, 32, 40, 48)
    v = V(1, 2, 3, 4, 5)  # the five fields a caller of the shorter struct sets: no run
    assert not v.mem and v.mem_start is None and v.nmem == 0


def test_header_declares_the_runs_and_no_new_entry_point():
    text = open(os.path.join(ROOT, "include", "lsmblk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\}\s*lsmblk_lsm_view;", header)
    fields = [re.sub(r"\s+", " ", f).strip() for f in m.group(1).split(";") if f.strip()]
    assert fields[-3:] == ["const lsmblk_kv_stream* mem", "const uint32_t* mem_start", "uint32_t nmem"]
    assert re.search(r"#define\s+LSMBLK_ABI_VERSION\s+1\b", header)
    assert "stay on the host" not in text
    names = set(re.findall(r"\b(lsmblk_\w+)\s*\(", header))
    assert names == {n for n, _, _ in _lib.SIGNATURES}  # the runs travel in the view: no entry point was added
    assert len(_lib.SIGNATURES) == 69
