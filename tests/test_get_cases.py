"""CPU: the generators of get_cases.py reach the input classes they were built for (fixed seeds), and
the restated read agrees with the pieces of it the oracle already has.  No GPU, no device call."""
import pytest

import get_cases as gc
from oracle import pyref


@pytest.fixture(scope="module")
def cls():
    return {n: gc.classes(n) for n in gc.CASES}


@pytest.mark.parametrize("name", ["bs128", "bs256"])
def test_small_blocks_reach_every_version_class(cls, name):
    c, n = gc.case(name), cls[name]
    assert all(s.bs == int(name[2:]) and 16 << 10 < len(s.buf) < 128 << 10 for s in c.ssts)
    assert n["land_not_first"] >= 500   # reference landings past a key's first version
    assert n["modes_differ"] >= 500     # lookups where default and MVCC disagree
    assert n["mvcc_cross"] >= 50        # MVCC walks that end in a later block than they began
    assert n["spill"] >= 200            # unfiltered spills to the next block
    assert n["end_invalid"] >= 1        # iterators ended after the last block
    assert min(n["found"], n["tombstone"], n["invisible"]) >= 200
    assert n["bloom_out"] >= 1500 and n["range_out"] >= 1
    assert n["image_tie"] == 0          # short keys: the images decide alone


def test_blocks_that_start_with_the_previous_blocks_key(cls):
    assert cls["bs128"]["dup_first"] > 200 and cls["ties"]["dup_first"] > 200


def test_some_absent_key_passes_the_bloom_filter(cls):
    """The single-version SST has 10 filter bits per key: ~1 % of its absent keys pass."""
    assert 1 <= cls["bs256"]["bloom_false_pos"] < 100
    assert cls["bs256"]["bloom_out"] > 2000


def test_image_ties_need_whole_keys(cls):
    c = gc.case("ties")
    assert all(len(fk) > gc.IMG_BYTES for fk in c.ssts[0].first_keys)
    assert len({gc.image(fk) for fk in c.ssts[0].first_keys}) == 1 < len(set(c.ssts[0].first_keys))
    # the third SST: first keys shorter than, as long as and longer than the image, 14 bytes shared
    lens = {len(fk) for fk in c.ssts[2].first_keys}
    assert min(lens) < gc.IMG_BYTES < max(lens) and gc.IMG_BYTES in lens
    assert cls["ties"]["image_tie"] > 500


def test_threshold_case_has_blocks_on_both_sides(cls):
    n = cls["threshold"]
    assert n["at_lds"] == 1 and n["big_block"] == 3
    c = gc.case("threshold")
    sizes = [end - 4 - off for (off, _, _), end in zip(c.ssts[0].metas, c.ssts[0].ends)]
    assert gc.kGetLdsBlock in sizes and gc.kGetLdsBlock + 1 in sizes and max(sizes) > 2 * gc.kGetLdsBlock
    assert n["big_walk"] >= 1           # a walk that arrives in an oversized block from the block before
    assert n["found"] and n["tombstone"] and n["invisible"] and n["spill"]


def test_4096_blocks(cls):
    n = cls["bs4096"]
    assert all(s.bs == 4096 and len(s.blocks) > 20 for s in gc.case("bs4096").ssts)
    assert n["land_not_first"] > 100 and n["mvcc_cross"] >= 1 and n["spill"] >= 10 and n["end_invalid"] >= 1
    assert n["big_block"] == 0          # block_size 4096 stays on the LDS path (blocks of up to 4098 bytes)


@pytest.mark.parametrize("name", gc.CASES)
def test_case_sizes_and_restated_read(name):
    c = gc.case(name)
    assert 2 <= len(c.ssts) <= 4 and len(c.keys) <= 8192
    exp, values, val_off = gc.expected(name, True, False)
    files, fo = c.files, c.file_off
    for i in range(0, len(c.keys), 7):
        s = c.ssts[c.q_sst[i]]
        b, e = gc.seek_to_key_inner(s, c.keys[i], False)
        assert (b, e) == (int(exp["blk"][i]), int(exp["ent"][i]))
        # the landing block's search is BlockIterator::seek_to_key over the block's own bytes
        p = max(sum(fk <= c.keys[i] for fk in s.first_keys) - 1, 0)
        ents = pyref.block_entries(s.buf[s.metas[p][0]:s.ends[p] - 4])
        assert gc.block_seek(ents, c.keys[i]) == (e if b == p else len(ents))
        if exp["status"][i] == gc.FOUND:
            vp, vl = int(exp["val_pos"][i]), int(exp["vlen"][i])
            assert files[vp:vp + vl] == values[i] and val_off[i + 1] - val_off[i] == vl
            assert s.blocks[int(exp["hit_blk"][i])][int(exp["hit_ent"][i])][1] <= c.read_ts[i]
        else:
            assert values[i] is None and val_off[i + 1] == val_off[i]
    assert fo[-1] == len(files)
