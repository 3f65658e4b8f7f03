"""The block-rule cases (block_rule_cases.py) do what they were built for: the oracle decodes both
base blocks to their entries and refuses every variant, every rule has a variant in both sizes, the
base blocks sit on the valid side of the rules they are meant to touch, and the broken entry is on
the path of the seek that looks for it."""
import pytest

import block_rule_cases as brc
from oracle import oracle as O


@pytest.mark.parametrize("name", brc.NAMES)
def test_oracle_verdict(name):
    c = brc.case(name)
    rc, ents = brc.verdict(name)
    if c.rule is None:
        assert rc == O.ORC_OK and ents == brc.base_entries(c.size)
    else:
        assert rc == O.ORC_E_MALFORMED


def test_every_rule_has_a_case_in_both_sizes():
    for size in brc.SIZES:
        have = {c.rule for c in brc.cases() if c.size == size}
        assert have == {None} | (set(brc.RULES) - set(brc.RAW_RULES)), (size, have)
    assert {c.rule for c in brc.cases() if c.size == "raw"} == set(brc.RAW_RULES)


@pytest.mark.parametrize("size", brc.SIZES)
def test_base_blocks(size):
    blk = brc.base_block(size)
    n, data_end, fks, offs = brc.layout(blk)
    assert n == len(brc.base_entries(size)) == (5 if size == "small" else 70)
    if size == "small":
        assert 100 <= len(blk) <= 120 and len(blk) <= brc.kGetLdsBlock
    else:
        assert len(blk) > brc.STAGING_LIMIT
    assert brc.u16(blk, offs[1]) == fks                      # p == fks: the valid side of `prefix`
    last = offs[-1]
    s = brc.u16(blk, last + 2)
    assert brc.u16(blk, last + 12 + s) == 0 and last + 14 + s == data_end  # the valid side of both length rules
    assert brc.BROKEN[size] == (n // 2 if size == "small" else 67)


@pytest.mark.parametrize("name", [c.name for c in brc.cases() if c.broken is not None])
def test_the_broken_entry_is_on_the_seek_path(name):
    c = brc.case(name)
    ents = brc.base_entries(c.size)
    assert ents[c.broken][0] == c.seek_key
    path = brc.seek_path(len(ents), c.broken)
    assert path[-1] == c.broken
    if c.size == "small" and c.broken == brc.BROKEN["small"]:
        assert path == [c.broken]  # the first probe
    if c.size == "big" and c.broken == 67:
        assert path == [35, 53, 62, 66, 68, 67]
    assert O.seek_key(brc.base_block(c.size), c.seek_key) == c.broken


@pytest.mark.parametrize("size", brc.SIZES)
def test_the_base_block_is_the_victim_tables_one_block(size):
    files, file_off, pos = brc.sst_pair(size)
    blk = brc.base_block(size)
    assert files[pos:pos + len(blk)] == blk and len(file_off) == 3
