"""The SST container inputs of tests/sst_cases.py, checked on the CPU: every generator must reach
the lengths, paths and threshold sides it was built for (under nominal addresses), and the
product's host pieces that share code with the kernels (fingerprint32) are compared with the
oracle on the same keys.  test_gpu_sst_paths.py runs the same inputs on the device."""
import numpy as np
import pytest

import sst_cases as sc
from lsm_amd import sst as S
from oracle import oracle as O
from oracle import pyref


def test_constants_are_read_from_the_kernel_sources(tmp_path):
    c = sc.C
    assert c.kBloomLds % 4 == 0 and c.kCrcChunk <= c.lds_chunk < c.kBloomLds and c.kCrcPad >= c.kCrcSeg
    assert c.kMetaTile == 256 and c.kMetaImg % 16 == 0
    f = tmp_path / "k.hip"
    f.write_text("constexpr uint32_t kBloomLdsX = 1;\n")
    with pytest.raises(RuntimeError):
        sc.kernel_constants({"kBloomLds": str(f)})


def test_a_retuned_constant_fails_the_checks(tmp_path):
    """Cases built for today's constants miss the targets of retuned ones: the checks notice."""
    import os
    def retuned(name, value):
        src = os.path.join(sc._CSRC, sc.SOURCES[name])
        text = open(src).read().replace(f"{name} = {getattr(sc.C, name)};", f"{name} = {value};")
        f = tmp_path / (name + ".src")
        f.write_text(text)
        c = sc.kernel_constants({name: str(f)})
        assert getattr(c, name) == value
        return c
    counts = sc.bloom_counts()
    for name, value in (("kBloomLds", sc.C.kBloomLds - 1024), ("kCrcSeg", sc.C.kCrcSeg + 4),
                        ("kCrcChunk", sc.C.kCrcChunk + 256)):
        c = retuned(name, value)
        with pytest.raises(AssertionError):
            sc.check_bloom_counts(counts, c)
        sc.check_bloom_counts(sc.bloom_counts(c), c)   # the probes follow the constant
    case, seg_blk = sc.meta_stream()
    lay = sc.layout(case)
    c = retuned("kMetaImg", sc.C.kMetaImg + 64)
    with pytest.raises(AssertionError):
        sc.check_meta_stream(case, seg_blk, lay, 0, c)
    case, seg_blk = sc.meta_stream(c=c)
    sc.check_meta_stream(case, seg_blk, sc.layout(case), 0, c)


def test_fingerprint_stream_lengths_and_host_hash():
    case = sc.fingerprint_stream()
    sc.check_fingerprint_stream(case)
    keys = [k for k, _, _ in sc.entries_of(case)]
    assert [S.fingerprint32(k) for k in keys] == [pyref.fingerprint32(k) for k in keys]
    for last in sc.fp_last_indices(case):
        moved, perm = sc.reorder_last(case, last)
        assert moved.tag[-1] == case.tag[last] and moved.kv.entry(moved.kv.n - 1) == case.kv.entry(last)
        assert sorted(perm.tolist()) == list(range(case.kv.n))


def test_bloom_counts_sit_on_the_switch_and_the_chunk_edges():
    counts = sc.bloom_counts()
    sc.check_bloom_counts(counts)
    if (sc.C.kBloomLds, sc.C.kCrcSeg, sc.C.kCrcChunk) == (32768, 68, 4096):  # today's values, by hand
        assert counts["lds"] == [3480, 3481, 6961, 6962, 6963, 10443, 10444, 10445, 26213]
        assert [sc.bloom_len(n) for n in counts["lds"]] == [4351, 4353, 8703, 8704, 8705, 13055, 13056, 13058, 32768]
        assert counts["global"] == [26214, 29489, 29490, 29491, 32766, 32767, 32768]
        assert [sc.bloom_len(n) for n in counts["global"]] == [32769, 36863, 36864, 36865, 40959, 40960, 40961]
    print({g: [(n,) + sc.bloom_path(n) for n in ns] for g, ns in counts.items()})


def test_bloom_lengths_are_the_oracles():
    """bloom_len (the classifier) against pyref.Bloom's own encoding, and the sections' sizes of
    layout() against pyref.sst_file's footers."""
    for n in (1, 6, 7, 8, 100, 3480, 3481):
        b = pyref.Bloom.build_from_key_hashes(list(range(n)), pyref.Bloom.bloom_bits_per_key(n, 0.01))
        assert len(b.filter) + 1 == sc.bloom_len(n), n
    case = sc.bloom_stream("min")
    lay = sc.layout(case)
    for s, want in enumerate(sc.expected_files(case)):
        assert len(want) == lay.file_len[s]
        assert int.from_bytes(want[-4:], "big") == lay.bloom_off[s]
        assert int.from_bytes(want[lay.bloom_off[s] - 4:lay.bloom_off[s]], "big") == lay.data_len[s]
    keys = [k for k, _, _ in sc.entries_of(case)]
    assert keys == sorted(set(keys)) and {len(k) for k in keys} <= set(range(8, 41))


def test_bloom_global_stream_steers_the_bloom_address():
    case = sc.bloom_stream("global")
    lay = sc.layout(case)
    dsh = sc.check_bloom_global(case, lay)
    kl = np.diff(case.kv.key_off.astype(np.int64))
    big = kl[kl != 5]
    assert big.min() == 8 and big.max() == 40 and (big > 24).sum() > len(big) // 3
    assert [n for n in case.tag if n] == sc.bloom_counts()["global"]
    print(f"global: {[n for n in case.tag if n]} keys, dsh {dsh}")


def test_layout_stream_conditions():
    case = sc.layout_stream()
    lay = sc.layout(case)
    sc.check_layout_stream(case, lay)
    want = sc.expected_files(case)
    assert [len(w) for w in want] == lay.file_len.tolist()


def test_capacity_streams_start_unaligned():
    for which in ("layout", "global"):
        case = sc.capacity_stream(which)
        lay = sc.layout(case)
        assert lay.file_off[1] & 3 == 1 and case.ent[1] == 1
        if which == "layout":
            assert len(case.ent) - 1 == sc.LAYOUT_ROUND + 2
        else:
            assert sc.bloom_path(int(case.ent[2] - case.ent[1]))[0] == "global" and bloom_dsh(lay, 1) != 0
    assert sc.bloom_path(sc.max_lds_count())[0] == "lds" and sc.bloom_path(sc.max_lds_count() + 1)[0] == "global"


def bloom_dsh(lay, s):
    return int(sc.bloom_addr(lay, s)) & 3


def test_meta_stream_conditions():
    for addr in (0, 5, 10):
        for empty in (True, False):
            case, seg_blk = sc.meta_stream(addr, empty_segments=empty)
            lay = sc.layout(case)
            t = sc.check_meta_stream(case, seg_blk, lay, addr)
            assert (np.diff(seg_blk.astype(np.int64)) == 0).sum() == (3 if empty else 0)
    print(sc.meta_coverage("meta @0", t))
    # the records' sizes of layout() are pyref's
    metas = sc.expected_metas(case, seg_blk)
    assert sum(len(m) for m in metas) == int(lay.rec.sum()) + 16 * (len(seg_blk) - 1)


def test_seek_cases_conditions():
    for bs in (1024, 4096):
        c = sc.seek_prefix_case(bs)
        p = c.prefix_lens()
        assert 0 in p and 1 in p and len(set(p[p >= 20].tolist())) >= 40, sorted(set(p.tolist()))
        print(sc.seek_coverage(f"prefix {bs}", c))
    c = sc.seek_chain_case(4096)
    keys = [c.kv.entry(i)[0] for i in range(c.kv.n)]
    deep = max(sum(1 for j in range(i) if keys[i].startswith(keys[j])) for i in range(len(keys)))
    assert deep >= 29
    c = sc.seek_big_case()
    cnt = [int.from_bytes(c.block(b)[-2:], "big") for b in range(len(c.blk_off) - 1)]
    assert cnt[0] > 2000 and len(c.block(0)) > 60000
    c = sc.seek_tiny_case()
    assert [int.from_bytes(c.block(b)[-2:], "big") for b in range(len(c.blk_off) - 1)] == [1, 2] * 13
    # a probe that must land on its own entry does so in the oracle
    want = c.expected()
    assert all(w == s for w, s in zip(want, c.q_self) if s >= 0)
