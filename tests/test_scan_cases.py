"""The range-scan cases (scan_cases.py) reach what they were built for, and the read filter's
predecessor-only closed form equals LsmIterator restated line by line -- CPU only."""
import numpy as np
import pytest

import scan_cases as sc


@pytest.mark.parametrize("name", sc.CASES)
def test_every_bound_kind_pair_occurs(name):
    c = sc.case(name)
    assert {(a, b) for a, b in zip(c.lkind, c.ukind)} == {(a, b) for a in sc.KINDS for b in sc.KINDS}
    assert any(lk and uk and lo == up for lk, lo, uk, up in zip(c.lkind, c.lower, c.ukind, c.upper))


def test_classes_are_reached():
    total = dict.fromkeys(sc.CLASSES, 0)
    per_case = {}
    for name in sc.CASES:
        for no_filter, mvcc in sc.MODES:
            n = sc.classes(name, no_filter, mvcc)
            per_case[name, no_filter, mvcc] = n
            for k, v in n.items():
                total[k] += v
    assert all(v >= 1 for v in total.values()), total
    for no_filter, mvcc in sc.MODES:  # what each case is for, in every mode
        assert per_case["ties", no_filter, mvcc]["end_image_tie"] >= 1
        t = per_case["threshold", no_filter, mvcc]
        assert t["big_first"] >= 1 and t["big_last"] >= 1 and t["excl_cross"] >= 1
        assert per_case["many_blocks", no_filter, mvcc]["ge65_blocks"] >= 1
        assert per_case["bs128", no_filter, mvcc]["lower_gt_upper"] >= 1
        assert per_case["bs128", no_filter, mvcc]["begin_differs"] >= 1
    assert per_case["bs128", False, False]["range_out"] >= 1 and per_case["bs128", True, False]["range_out"] == 0


def test_many_blocks_touch_counts_and_query_counts():
    c = sc.case("many_blocks")
    assert len(c.ssts[0].blocks) >= 200 and len(c) >= max(sc.query_counts())
    for mode in sc.MODES:
        exp, _ = sc.expected("many_blocks", *mode)
        got = set(exp["blocks"].tolist())
        assert set(sc.MANY_TOUCH) <= got and max(got) == len(c.ssts[0].blocks), sorted(got)[-5:]


def test_threshold_ranges_cover_the_lds_threshold_blocks():
    c = sc.case("threshold")
    s = c.ssts[2]
    sizes = [end - 4 - off for (off, _, _), end in zip(s.metas, s.ends)]
    want = {sc.kGetLdsBlock, sc.kGetLdsBlock + 1, 3 * sc.kGetLdsBlock}
    assert want <= set(sizes)
    exp, _ = sc.expected("threshold", True, False)
    for z in want:  # a range begins at, ends with and passes through each of them
        b = sizes.index(z)
        sel = [i for i in range(len(c)) if c.q_sst[i] == 2 and exp["n"][i]]
        last = lambda i: int(exp["blk1"][i]) - (0 if exp["ent1"][i] else 1)
        assert any(exp["blk0"][i] == b and last(i) > b for i in sel), z
        assert any(last(i) == b and exp["blk0"][i] < b for i in sel), z
        assert any(exp["blk0"][i] < b < last(i) for i in sel), z


def test_expectation_agrees_with_a_sorted_slice():
    """On these builder-written SSTs the MVCC-mode range is the slice of the entries by key."""
    for name in ("bs256", "threshold"):
        c = sc.case(name)
        _, rows = sc.expected(name, True, True)
        for si, lk, lo, uk, up, got in zip(c.q_sst, c.lkind, c.lower, c.ukind, c.upper, rows):
            if (lk and not lo) or (uk and not up):
                continue
            want = [e for e in c.ssts[si].entries
                    if (lk == 0 or (e[0] >= lo if lk == 1 else e[0] > lo)) and (uk == 0 or (e[0] <= up if uk == 1 else e[0] < up))]
            assert got == want


@pytest.mark.parametrize("name", sc.CASES)
def test_read_filter_rule_equals_lsm_iterator(name):
    c = sc.case(name)
    for mode in ((True, False), (True, True)):
        _, rows = sc.expected(name, *mode)
        seen = set()
        for r in rows:
            key = (len(r), r[0] if r else None, r[-1] if r else None)
            if key in seen or len(r) > 400:
                continue
            seen.add(key)
            for ts in sc.read_ts_values(c):
                assert sc.read_filter_rule(r, ts) == sc.lsm_iterate(r, ts), (name, mode, ts)
    whole = c.ssts[0].entries  # and one whole table
    for ts in sc.read_ts_values(c):
        assert sc.read_filter_rule(whole, ts) == sc.lsm_iterate(whole, ts)


def test_read_filter_rule_needs_newest_first():
    """Versions not newest first: the loop and the closed form differ, so the check above can fail."""
    ents = [(b"k", 5, b"old"), (b"k", 9, b"new"), (b"m", 1, b"x")]
    assert sc.lsm_iterate(ents, 7) == [(b"k", 5, b"old"), (b"m", 1, b"x")]
    assert sc.read_filter_rule(ents, 7) == [(b"k", 5, b"old"), (b"m", 1, b"x")]
    ents = [(b"k", 5, b"old"), (b"k", 9, b"new"), (b"k", 6, b"mid"), (b"m", 1, b"x")]
    assert sc.lsm_iterate(ents, 7) == [(b"k", 5, b"old"), (b"m", 1, b"x")]
    assert sc.read_filter_rule(ents, 7) == [(b"k", 5, b"old"), (b"k", 6, b"mid"), (b"m", 1, b"x")]


def test_lsm_iterator_first_position_quirk():
    """LsmIterator::new does not test its first position against the end bound; the per-SST scan does."""
    ents = [(b"b", 3, b"v"), (b"c", 3, b"w")]
    assert sc.lsm_iterate(ents, 10, (sc.EXCLUDED, b"a")) == [(b"b", 3, b"v")]
    s = sc.case("bs256").ssts[0]
    k = s.entries[10][0]
    assert sc.scan_one(s, sc.INCLUDED, k, sc.EXCLUDED, k, True, False)["n"] == 0
