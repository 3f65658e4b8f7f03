"""The path-coverage inputs of tests/path_cases.py, checked on the CPU: every generator's stream
is oracle-encoded, classified under nominal addresses (aligned bases plus the chosen shift), and
must reach the paths and threshold sides it was built for; and decode(encode(kv)) == kv on the
oracle, as a check of the generator itself.  test_gpu_paths.py runs the same inputs on the device."""
import numpy as np
import pytest

import path_cases as pc
from oracle import oracle as O

CUS = 256  # an MI355X; the GPU tests re-assert everything for the device they run on


def encode(case):
    kv, seg, bs = case[:3]
    rc, blocks, off = O.encode_segments(kv, seg, bs)
    assert rc == 0
    rc, back = O.decode_blocks(blocks, off)
    assert rc == 0 and pc.kv_equal(back, kv), "generator: the oracle does not read its own blocks back"
    return kv, seg, blocks, off


def probe(case):
    kv, seg, blocks, off = encode(case)
    assert pc.one_block_per_segment(off, seg), (len(off) - 1, len(seg) - 1)
    return kv, seg, blocks, off


def test_constants_are_read_from_the_kernel_source(tmp_path):
    assert set(pc.K) == set(pc._NAMES) and all(v > 0 for v in pc.K.values())
    assert pc.kDecOut < pc.kDecImg and pc.kEmitKCap < pc.kEmitICap and pc.kTile == 64
    f = tmp_path / "k.hip"
    f.write_text("constexpr uint32_t kDecImg = 1;\n")
    with pytest.raises(RuntimeError):
        pc.kernel_constants(str(f))


def test_wave_sequences_strided_assignment():
    big = np.array([1, 0, 0, 1, 1, 0, 0], bool)
    assert pc.wave_sequences(big, 3) == ["BBF", "FB", "FF"]
    assert pc.wave_sequences(big, 16) == list("BFFBBFF")


def test_stream_a_conditions():
    kv, seg, bs = pc.stream_a(CUS)
    assert len(seg) - 1 > 64 and len(set(np.diff(seg.astype(np.int64)))) > 32
    kv, seg, blocks, off = encode((kv, seg, bs))
    assert 30e6 < len(blocks) < 60e6
    p = pc.classify(blocks, off, kv.key_off, kv.val_off)
    pc.check_stream_a(p, CUS)
    print(pc.coverage_line("A", p))


def test_stream_b_conditions():
    kv, seg, bs = pc.stream_b(CUS)
    kv, seg, blocks, off = encode((kv, seg, bs))
    p = pc.classify(blocks, off, kv.key_off, kv.val_off)
    pc.check_stream_b(p, CUS)
    d = p.dec_counts()
    assert d["staged-simple"] > 0 and d["big-tables"] > 0 and d["fast-lds"] > 0
    print(pc.coverage_line("B", p))


def test_probes_emit_count():
    kv, seg, blocks, off = probe(pc.probes_emit_count())
    p = pc.classify(blocks, off, kv.key_off, kv.val_off)
    assert tuple(p.n) == pc.EMIT_COUNT_NS
    assert pc.both_sides(p.lhs_n, pc.kEmitMaxE)
    np.testing.assert_array_equal(p.fail, np.where(p.n > pc.kEmitMaxE, pc.FAIL_N, 0))
    print(pc.coverage_line("emit count", p))


def test_probes_emit_keycap():
    kv, seg, blocks, off = probe(pc.probes_emit_keycap())
    seen = {}
    for shift in range(16):
        p = pc.classify(blocks, off, kv.key_off, kv.val_off, key_addr=256 + shift)
        assert (p.n == 20).all() and ((p.fail & ~pc.FAIL_K) == 0).all()
        KB = p.lhs_k - p.klead - 8
        assert set(KB) == set(range(pc.kEmitKCap - 40, pc.kEmitKCap + 9))
        for kl, lhs in zip(p.klead, p.lhs_k):
            seen.setdefault(int(kl), set()).add(int(lhs))
    for kl in range(16):
        assert {pc.kEmitKCap, pc.kEmitKCap + 1} <= seen[kl], kl


def test_probes_emit_valcap_and_size_cap_single_entry():
    kv, seg, blocks, off = probe(pc.probes_emit_valcap())
    lv, ls, alone = set(), set(), 0
    for shift in range(16):
        p = pc.classify(blocks, off, kv.key_off, kv.val_off, val_addr=256 + shift)
        assert (p.n == 1).all() and ((p.fail & (pc.FAIL_N | pc.FAIL_K)) == 0).all()
        lv |= set(p.lhs_v.tolist())
        ls |= set(p.lhs_s.tolist())
        # the value cap alone: it fails, the size cap holds
        m = p.fail == pc.FAIL_V
        assert (p.vlead[m] >= p.olead[m] + 4).all()
        alone += int(m.sum())
        if shift == 0:
            print(pc.coverage_line("emit valcap", p))
    want = set(range(pc.kEmitICap - 17, pc.kEmitICap + 18))
    assert want <= lv and want <= ls
    assert alone > 0


def test_probes_emit_sizecap_multi_entry():
    kv, seg, blocks, off = probe(pc.probes_emit_sizecap())
    p = pc.classify(blocks, off, kv.key_off, kv.val_off)
    assert (p.n == 20).all() and ((p.fail & ~pc.FAIL_S) == 0).all()
    assert p.lhs_k.max() <= pc.kEmitKCap - 40 and p.lhs_v.max() <= pc.kEmitICap - 1000  # only the size cap is near
    assert set(range(pc.kEmitICap - 17, pc.kEmitICap + 18)) <= set(p.lhs_s.tolist())
    print(pc.coverage_line("emit sizecap", p))


def test_probes_decode_staged_edge():
    kv, seg, blocks, off = probe(pc.probes_dec_staged())
    ln = np.diff(off.astype(np.int64))
    seen = {}
    for shift in range(16):
        p = pc.classify(blocks, off, kv.key_off, kv.val_off, blk_addr=256 + shift)
        for n in (1, 2, 128):
            m = p.n == n
            assert sorted(ln[m]) == list(pc.DEC_STAGED_LENS), n
            lead = p.lhs_img[m] - ln[m] - 15
            for ld, lhs in zip(lead, p.lhs_img[m]):
                seen.setdefault((n, int(ld)), set()).add(int(lhs))
            # fast up to the edge (the long values of 1 and 2 entries through the global sink), the
            # tables path beyond it
            assert set(p.dec[m]) == ({0, 3} if n == 128 else {1, 3}), (n, set(p.dec[m]))
    for n in (1, 2, 128):
        for ld in range(16):
            assert {pc.kDecImg, pc.kDecImg + 1} <= seen[(n, ld)], (n, ld)
    print(pc.coverage_line("decode staged", p))


def test_probes_decode_entry_count():
    kv, seg, bs, nstaged = pc.probes_dec_count()
    kv, seg, blocks, off = probe((kv, seg, bs))
    p = pc.classify(blocks, off, kv.key_off, kv.val_off)
    want_staged = [n for n in pc.DEC_COUNT_NS if n <= pc.DEC_COUNT_STAGED_MAX]
    assert sorted(p.n[:nstaged]) == want_staged and tuple(p.n[nstaged:]) == pc.DEC_COUNT_NS
    # every count but 257 exists staged: 257 entries take 257 x 16 + 3 bytes at the least
    assert [n for n in pc.DEC_COUNT_NS if n not in want_staged] == [257] and 257 * 16 + 3 + 15 > pc.kDecImg
    for b in range(len(p.n)):
        small = p.n[b] <= pc.kDecMaxE
        if b < nstaged:
            assert pc.DEC_PATHS[p.dec[b]] == ("fast-lds" if small else "staged-simple"), (b, p.n[b])
        else:
            assert p.lhs_img[b] > pc.kDecImg + 16 + 15
            assert pc.DEC_PATHS[p.dec[b]] == ("big-tables" if small else "big-chunked"), (b, p.n[b])
    print(pc.coverage_line("decode count", p))


def test_probes_decode_output_image():
    kv, seg, blocks, off = probe(pc.probes_dec_outimage())
    p = pc.classify(blocks, off, kv.key_off, kv.val_off)
    m = p.n == 30
    assert (p.dec[m] <= 1).all() and m.sum() * 2 == len(p.n)
    ko, vo = kv.key_off.astype(np.int64), kv.val_off.astype(np.int64)
    s = p.first[m]
    KV_ = (ko[s + 30] - ko[s]) + (vo[s + 30] - vo[s])
    assert set(range(pc.kDecOut - 48, pc.kDecOut + 17)) <= set(KV_.tolist())
    for kb in pc.OUT_LEADS:
        for vb in pc.OUT_LEADS:
            q = m & (p.kb == kb) & (p.vb == vb)
            assert pc.both_sides(p.lhs_out[q], pc.kDecOut, near=16), (kb, vb)
            assert {0, 1} <= set(p.dec[q])
    print(pc.coverage_line("decode outimage", p))
