"""The CRC inputs of tests/crc_cases.py, checked on the CPU: every generator must reach the lengths,
alignments, routes and errors it was built for (under nominal addresses and CU counts), a retuned
constant or a cut-down generator must fail those checks, the data must not hide an off-by-one, and
the two references (oracle.crc32, zlib) must agree.  test_gpu_crc_paths.py runs the same inputs on
the device."""
import os
import zlib

import numpy as np
import pytest

import crc_cases as cc
from oracle import oracle as O


def test_constants_are_read_from_the_kernel_sources(tmp_path):
    c = cc.C
    assert c.kCrcSeg % 4 == 0 and c.kCrcSeg <= c.kCrcPad and c.kCrcChunk + 3 <= 64 * c.kCrcSeg
    assert c.kCrcChunk % cc.LOAD_PIECE == 0 and c.kCsWaves * 64 <= 1024
    f = tmp_path / "k.hip"
    f.write_text("constexpr uint32_t kCsWavesX = 1;\n")
    with pytest.raises(RuntimeError):
        cc.kernel_constants({"kCsWaves": str(f)})


def test_a_retuned_constant_fails_the_checks(tmp_path):
    """Cases built for today's constants miss the targets of retuned ones, and the generators
    follow the constant."""
    def retuned(**values):
        paths = {}
        for name, value in values.items():
            src = paths.get(name, os.path.join(cc._CSRC, cc.SOURCES[name]))
            text = open(src).read().replace(f"{name} = {getattr(cc.C, name)};", f"{name} = {value};")
            f = tmp_path / (name + ".src")
            f.write_text(text)
            paths.update({n: str(f) for n, s in cc.SOURCES.items() if s == cc.SOURCES[name]})
        c = cc.kernel_constants(paths)
        assert all(getattr(c, name) == value for name, value in values.items())
        return c
    blocks = cc.block_case()
    # (a lane window over kCrcPad would read past the zero pad, so the two move together: the
    # +- 80 around a chunk edge holds every window edge of a kCrcSeg up to today's kCrcPad)
    for values in (dict(kCrcChunk=cc.C.kCrcChunk - 256), dict(kCrcSeg=100, kCrcPad=112)):
        c = retuned(**values)
        with pytest.raises(AssertionError):
            cc.check_block_case(blocks, c)
        cc.check_block_case(cc.block_case(c), c)   # the probes follow the constant
    c = retuned(kCrcPad=cc.C.kCrcSeg - 4)
    with pytest.raises(AssertionError):
        cc.check_block_case(blocks, c)
    nblk = cc.persistent_stream_nblk(cc.NOMINAL_CUS)
    for value in (cc.C.kCsWaves // 2, cc.C.kCsWaves * 2):
        c = retuned(kCsWaves=value)
        with pytest.raises(AssertionError):
            cc.check_persistent_stream(nblk, cc.NOMINAL_CUS, c)
        cc.check_persistent_stream(cc.persistent_stream_nblk(cc.NOMINAL_CUS, c), cc.NOMINAL_CUS, c)


def test_a_cut_down_generator_fails_the_checks():
    """Without the lengths around the first chunk edge, (a) no longer passes its check."""
    cut = [L for L in cc.stream_lengths() if abs(L - cc.STREAM_CHUNK) > 40]
    assert len(cut) == len(cc.stream_lengths()) - 81
    with pytest.raises(AssertionError, match="chunk edge 1"):
        cc.check_stream_case(cc.stream_case(lengths=cut))
    short = [L for L in cc.stream_lengths() if L >= 16]
    with pytest.raises((AssertionError, StopIteration)):
        cc.check_stream_case(cc.stream_case(lengths=short))


# ------------------------------------------------------------------------------- a
@pytest.mark.parametrize("tail", [0, 4])
def test_streaming_lengths_reach_every_tail_pad_and_chunk_edge(tail):
    r = cc.stream_case(tail)
    assert r.nblk == 550 + cc.EXTRA_EMPTY and sorted(r.lens().tolist()) == sorted(cc.stream_lengths() + [0] * cc.EXTRA_EMPTY)
    print(cc.check_stream_case(r))
    lens = r.lens()
    nz = np.flatnonzero(lens > 0)
    assert (r.body[r.off[:-1][nz]] != 0).all() and (r.body[r.off[:-1][nz] + lens[nz] - 1] != 0).all()
    if tail:
        gaps = np.concatenate([r.body[int(e) - tail:int(e)] for e in r.off[1:]])
        assert (gaps != 0).all()
    for n in cc.stream_counts(r.nblk):   # the cut batches are prefixes: the later blocks' bytes follow them
        p = r.prefix(n)
        assert p.nblk == n and p.body is r.body and cc.stream_waves(p.off, tail).nb[-1] == (n - 1) % 4 + 1


def test_streaming_expectation_is_the_oracles_and_zlibs():
    """(a)'s expected CRCs come from oracle.crc32; zlib gives the same on every block."""
    r = cc.stream_case()
    want, refused = cc.expected_crcs(r, O.crc32)
    assert not refused.any()
    assert want.tolist() == [zlib.crc32(r.block(b)) for b in range(r.nblk)]
    assert (want[r.lens() == 0] == 0).all() and (want[r.lens() > 0] != 0).all()


def test_placement_leaves_no_zero_outside_the_stream():
    r = cc.stream_case()
    for shift in (0, 7, 15):
        img, start = cc.placed(r.body, shift)
        assert start % 16 == shift and img[start:start + len(r.body)].tobytes() == r.body.tobytes()
        assert (img[:start] != 0).all() and (img[start + len(r.body):] != 0).all()
        assert start >= cc.GUARD and len(img) - start - len(r.body) >= cc.GUARD


@pytest.mark.parametrize("tail", [0, 4])
def test_streaming_data_does_not_hide_an_off_by_one(tail):
    r = cc.stream_case(tail)
    assert cc.sensitivity(r, cc.stream_edges) == [], "a zero byte on a probed position"


# ------------------------------------------------------------------------------- b
def test_streaming_persistent_loop_is_entered():
    nblk = cc.persistent_stream_nblk(cc.NOMINAL_CUS)
    print(cc.check_persistent_stream(nblk, cc.NOMINAL_CUS))
    for cus in (64, 228, 304):   # the device's own count is the GPU test's parameter
        cc.check_persistent_stream(cc.persistent_stream_nblk(cus), cus)
    with pytest.raises(AssertionError):   # the largest batch of the older CRC tests: one group per wave
        cc.check_persistent_stream(13000, cc.NOMINAL_CUS)
    r = cc.persistent_stream_case(64)
    assert r.nblk == cc.persistent_stream_nblk(64) and r.lens().min() == 0 and r.lens().max() == 40


# ------------------------------------------------------------------------------- c
def test_error_cases_take_the_fallback_and_name_the_refused():
    cases = cc.error_cases()
    print(cc.check_error_cases(cases))
    by = {ec.name: ec for ec in cases}
    for tail in (0, 4):
        for name, off in ((f"Se<S0 tail{tail}", [100, 200, 0, 50, 60]), (f"valid below S0 tail{tail}", [50, 100, 0, 200, 300])):
            ec = by[name]
            assert ec.off == off and not cc.stream_waves(ec.off, tail).wave_ok.any()
            _, refused = cc.expected_crcs(cc.error_ranges(ec))
            assert refused.tolist() == [False, True, False, False]
        ec = by[f"over 2 GiB last tail{tail}"]
        assert ec.off[-1] - ec.off[-2] == 0x7FFFFFF1 and ec.span == ec.off[-2]
        assert cc.expected_crcs(cc.error_ranges(ec))[1].tolist() == [False, False, True]
    for short in range(4):
        want, refused = cc.expected_crcs(cc.error_ranges(by[f"{short} bytes under tail 4"]))
        assert refused.sum() == 1 and want[refused][0] == 0 and int(np.flatnonzero(refused)[0]) % 4 == short
    want, refused = cc.expected_crcs(cc.error_ranges(by["4 bytes under tail 4"]))
    assert not refused.any() and want[5] == 0 and (np.delete(want, 5) != 0).all()


# ------------------------------------------------------------------------------- d, e
def test_one_entry_blocks_reach_every_lead_mask_and_window():
    case = cc.block_case()
    print(cc.check_block_case(case))
    fr = case.framed()
    assert fr.tail == 4 and (fr.lens() == case.lens()).all()
    for b in (0, fr.nblk // 2, fr.nblk - 1):
        blk = fr.block(b)
        assert blk == case.blocks[int(case.blk_off[b]):int(case.blk_off[b + 1])].tobytes()
        assert int.from_bytes(fr.body[int(fr.off[b + 1]) - 4:int(fr.off[b + 1])].tobytes(), "big") == zlib.crc32(blk)
    rc, kv = O.decode_blocks(case.blocks, case.blk_off)
    assert rc == 0 and cc.pc.kv_equal(kv, case.kv)


def test_block_data_does_not_hide_an_off_by_one():
    """(d) through both kernels' chunk edges.  An encoded block starts with its first entry's
    overlap, a zero u16: zeroing its first byte is the one vacuous mutant (the verifying decode's
    flip of that byte is what tests it on the device)."""
    case = cc.block_case()
    fr = case.framed()
    edges = lambda L: sorted(set(cc.stream_edges(L)) | set(cc.kernel_edges(L)))
    vac = cc.sensitivity(fr, edges)
    assert {b for b, i in vac if i == 0} == set(range(fr.nblk))
    klen = np.diff(case.kv.key_off.astype(np.int64))
    for b, i in vac:   # a one-entry block: overlap u16, klen's and vlen's high bytes
        if not isinstance(case.tag[b], tuple):
            assert i in (0, 1, 2, 12 + int(klen[int(case.seg[b])])), (b, i)


def test_persistent_kernel_takes_three_blocks_a_wave():
    for cus in (64, cc.NOMINAL_CUS, 304):
        print(cc.check_persistent_kernel(cc.persistent_kernel_nblk(cus), cus))
    with pytest.raises(AssertionError):
        cc.check_persistent_kernel(cc.persistent_kernel_nblk(cc.NOMINAL_CUS) // 2, cc.NOMINAL_CUS)
    case = cc.persistent_kernel_case(8)
    lens = case.lens()
    assert len(lens) == cc.persistent_kernel_nblk(8) and lens.min() >= 19 and lens.max() <= 60


# ------------------------------------------------------------------------------- f
def test_meta_sections_reach_every_lead_mask_and_window():
    case = cc.meta_case()
    print(cc.check_meta_case(case))
    sec = cc.meta_sections(case)
    for s in (0, len(sec) // 2, len(sec) - 1):
        assert int.from_bytes(sec[s][-4:], "big") == zlib.crc32(sec[s][4:-4]) and len(sec[s]) == case.region[s] + 8
    addr, lens = cc.meta_leads(case, 0x1000 + 5)
    assert addr[0] == 0x1000 + 5 + 4 and addr[1] == addr[0] + len(sec[0]) and lens.tolist() == case.region
