"""The CRC-32 kernels on the inputs of crc_cases.py: crc_stream_kernel through lsmblk_crc32_batch,
the framed encode and the lagged verifying decode; crc_kernel<true> (the fused count) through the
two-pass verifying decode; crc_kernel<false> through the BlockMeta sections.  Every test re-asserts
its coverage with the device's CU count and the tensors' addresses, then compares with zlib and
the oracle -- never with another call into the library."""
import zlib
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import crc_cases as cc
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch
from lsm_amd._lib import LSMBLK_DEBUG_TWO_PASS_DECODE, LSMBLK_E_CHECKSUM, LSMBLK_E_MALFORMED, LsmBlkError, lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A     # the crc tensor's guard words
CRC_GUARD = 4
TWO_PASS = LSMBLK_DEBUG_TWO_PASS_DECODE
MODES = ("lagged", "two_pass")   # crc_stream_kernel + the count pass; crc_kernel<true>'s fused count


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def to_device(body, shift, seed=0):
    """body on the device at an address `shift` mod 16, random non-zero bytes around it
    -> (whole image tensor, the stream's view, the host image, the stream's start in it)."""
    img, start = cc.placed(body, shift, seed)
    t = torch.from_numpy(img).cuda()
    view = t[start:start + len(body)]
    assert t.data_ptr() % 16 == 0 and view.data_ptr() % 16 == shift
    return t, view, img, start


def dev_off(off):
    return torch.from_numpy(np.ascontiguousarray(off, np.int64)).cuda()


def run_crc(view, off, tail):
    """lsmblk_crc32_batch -> (u32[nblk] CRCs, stats); the crc tensor's guard words must keep their fill."""
    nblk = len(off) - 1
    crc = torch.full((nblk + CRC_GUARD,), FILL, dtype=torch.int32, device="cuda")
    stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device="cuda")
    batch.crc32_into(view, dev_off(off), nblk, crc, stats, tail=tail)
    torch.cuda.synchronize()
    got = crc.cpu().numpy().view(np.uint32)
    assert (got[nblk:] == FILL).all(), "words after crc[nblk] written"
    return got[:nblk], stats.cpu().tolist()


def crc_check(r, view, want, what):
    got, st = run_crc(view, r.off, r.tail)
    bad = np.flatnonzero(got != want[:r.nblk])
    assert bad.size == 0, (f"{what}: {bad.size} CRCs differ, first block {int(bad[0])} of {int(r.lens()[bad[0]])} bytes: "
                           f"{int(got[bad[0]]):#x} for {int(want[bad[0]]):#x}")
    assert st[0] == r.nblk and st[1] == int(r.off[-1] - r.off[0]) and st[3] == 0, (what, st)


# ------------------------------------------------------------------------------- a
@pytest.mark.parametrize("tail", [0, 4])
def test_streaming_lengths_at_every_placement_and_batch_tail(tail):
    """(a): every length class at all 16 placements, the batch whole, cut to the other three
    residues mod 4 and as one block; tail 4: four random bytes after each block stay out of it."""
    r = cc.stream_case(tail)
    line = cc.check_stream_case(r)
    want, refused = cc.expected_crcs(r, O.crc32)
    assert not refused.any()
    for shift in range(16):
        _, view, _, _ = to_device(r.body, shift)
        for n in cc.stream_counts(r.nblk):
            crc_check(r.prefix(n), view, want, f"shift {shift}, {n} blocks")
    print(f"streaming lengths on {cu_count()} CUs, 16 placements x batches of {cc.stream_counts(r.nblk)}: {line}")


# ------------------------------------------------------------------------------- b
def test_streaming_persistent_loop():
    """(b): more than two groups per wave of the full grid, a partial last group."""
    cus = cu_count()
    r = cc.persistent_stream_case(cus)
    line = cc.check_persistent_stream(r.nblk, cus)
    want, _ = cc.expected_crcs(r)
    _, view, _, _ = to_device(r.body, 9)
    crc_check(r, view, want, "persistent stream")
    print("streaming persistent loop: " + line)


# ------------------------------------------------------------------------------- c
def test_streaming_fallback_and_error_contract():
    """(c): decreasing offsets, ranges under tail and over 2 GiB: the CRC of every valid range, 0
    and LSMBLK_ERR_MALFORMED for a refused one, stats[0] and stats[1] as for a clean batch."""
    cases = cc.error_cases()
    line = cc.check_error_cases(cases)
    fallback = 0
    for i, ec in enumerate(cases):
        r = cc.error_ranges(ec)
        want, refused = cc.expected_crcs(r)
        fallback += int((~cc.stream_waves(r.off, r.tail).wave_ok).sum())
        _, view, _, _ = to_device(r.body, i % 16)
        got, st = run_crc(view, r.off, r.tail)
        assert got.tolist() == want.tolist(), (ec.name, got, want)
        assert (got[refused] == 0).all()
        assert st[3] == (cc.ERR_MALFORMED if refused.any() else 0), (ec.name, st)
        assert st[0] == r.nblk and st[1] == int(r.off[-1] - r.off[0]), (ec.name, st)
    print(f"streaming errors: {line}; wave_ok == false waves {fallback}")


# ------------------------------------------------------------------------------- the framed encode
_cache = {}


def block_case():
    if "d" not in _cache:
        case = cc.block_case()
        rc, kv = O.decode_blocks(case.blocks, case.blk_off)
        assert rc == 0
        cnt = cc.pc.block_entry_counts(case.blocks, case.blk_off.astype(np.int64))
        _cache["d"] = (case, case.framed(), kv, np.concatenate([[0], np.cumsum(cnt)]))
    return _cache["d"]


def kv_to_dev(kv):
    return batch.KVStream.from_numpy(kv.keys, kv.key_off, kv.vals, kv.val_off, kv.ts)


def encode_raw(d, seg, bs, framed, slots=False, fill=0xA5):
    """encode_into over an output filled with `fill` -> (status, out, blk_off, seg_out, stats)."""
    kb, vb = d.byte_sizes()
    cap, blk_cap = batch.encode_bound(d, kb, vb, framed=framed)
    out = batch._aligned_empty(cap, "cuda")
    out.fill_(fill)
    off = torch.zeros(blk_cap, dtype=torch.int64, device="cuda")
    st = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device="cuda")
    seg_t = batch._u32_table(np.asarray(seg, np.uint32), out.device)
    so = torch.zeros(2 * (len(seg) - 1), dtype=torch.int64, device="cuda") if slots else None
    batch.encode_into(d, seg_t, len(seg) - 1, bs, out, cap, off, blk_cap, st, seg_out=so, framed=framed)
    torch.cuda.synchronize()
    return batch._status(st), out, off, so, st.cpu().tolist()


def test_framed_encode_blocks_and_crcs():
    """The framed encode's CRC route (the plan's block sizes, CRCs written big-endian after each
    block, the block count read on the device) over (d): every block the oracle's, the four bytes
    after it zlib's CRC of the oracle's block; with slots nothing else of the output changes."""
    case, fr, _, _ = block_case()
    cc.check_block_case(case)
    d = kv_to_dev(case.kv)
    status, out, off, _, st = encode_raw(d, case.seg, case.bs, framed=True)
    assert status == 0 and st[0] == fr.nblk and st[1] == len(fr.body)
    assert off[:fr.nblk + 1].cpu().numpy().tolist() == fr.off.tolist()
    got = out.cpu().numpy()
    for b in np.flatnonzero([got[int(fr.off[b]):int(fr.off[b + 1])].tobytes() != fr.body[int(fr.off[b]):int(fr.off[b + 1])].tobytes()
                             for b in range(fr.nblk)]):
        blk = got[int(fr.off[b]):int(fr.off[b + 1]) - 4].tobytes()
        what = "block" if blk != fr.block(b) else "CRC"
        pytest.fail(f"packed: {what} of block {b} ({len(blk)} bytes) differs")
    status, out, off, so, st = encode_raw(d, case.seg, case.bs, framed=True, slots=True)
    assert status == 0 and st[0] == fr.nblk
    s = case.seg.astype(np.int64)
    ko, vo = case.kv.key_off.astype(np.int64), case.kv.val_off.astype(np.int64)
    slot = ko[s[:-1]] + vo[s[:-1]] + 22 * s[:-1]
    so = so.cpu().numpy().reshape(-1, 2)
    assert so[:, 0].tolist() == slot.tolist() and so[:, 1].tolist() == np.diff(fr.off).tolist()
    want = np.full(out.numel(), 0xA5, np.uint8)
    for b in range(fr.nblk):   # one block per segment
        want[int(slot[b]):int(slot[b]) + int(so[b, 1])] = fr.body[int(fr.off[b]):int(fr.off[b + 1])]
    bad = np.flatnonzero(out.cpu().numpy() != want)
    assert bad.size == 0, f"slots: {bad.size} bytes differ, the first at {int(bad[0])}"
    lens = case.lens()
    print(f"framed encode: {fr.nblk} blocks of {int(lens.min())}..{int(lens.max())} bytes, packed and in slots")


@pytest.mark.parametrize("what", ["empty_key", "val_off"])
def test_refused_framed_encode_writes_nothing(what):
    """A refused encode leaves the framed packed output as it was (no CRC bytes either: the CRC
    pass reads a block count of zero) and reports what the packed mode reports."""
    ents = [(b"k%05d" % i, i, b"v" * 40) for i in range(600)]
    if what == "empty_key":
        ents[300] = (b"", 300, b"v" * 40)
    d = kv_to_dev(O.KV.from_entries(ents))
    if what == "val_off":
        d.val_off[301] = d.val_off[299]  # entry 300 ends before it starts
    seg = [0, 250, 600]
    plain, out, _, _, _ = encode_raw(d, seg, 4096, framed=False)
    assert plain != 0 and bool((out == 0xA5).all())
    status, out, _, _, _ = encode_raw(d, seg, 4096, framed=True)
    assert status == plain
    assert bool((out == 0xA5).all())


# ------------------------------------------------------------------------------- the verifying decode
@contextmanager
def decode_mode(mode):
    ctx = batch._ctx(0)
    assert lib().lsmblk_debug_set(ctx, TWO_PASS, int(mode == "two_pass")) == 0
    try:
        yield
    finally:
        lib().lsmblk_debug_set(ctx, TWO_PASS, 0)


def assert_kv_equal(dkv, ref):
    keys, ko, vals, vo, ts = dkv.to_numpy()
    assert dkv.n == ref.n
    np.testing.assert_array_equal(ko, ref.key_off)
    np.testing.assert_array_equal(vo, ref.val_off)
    np.testing.assert_array_equal(ts, ref.ts)
    np.testing.assert_array_equal(keys, ref.keys[:ref.key_off[-1]])
    np.testing.assert_array_equal(vals, ref.vals[:ref.val_off[-1]])


def decode_check(view, off, kv, ent):
    got, e = batch.decode_blocks(view, off, tail=4, verify=True, with_blk_ent=True)
    assert_kv_equal(got, kv)
    np.testing.assert_array_equal(e.cpu().numpy(), ent)


def decode_status(view, off):
    try:
        batch.decode_blocks(view, off, tail=4, verify=True)
    except LsmBlkError as e:
        return e.status
    return 0


@pytest.mark.parametrize("mode", MODES)
def test_verifying_decode_at_every_placement(mode):
    """(d) framed at all 16 placements: the oracle's stream and block entry index, no flag."""
    case, fr, kv, ent = block_case()
    lens = case.lens()
    sets = []
    off = dev_off(fr.off)
    with decode_mode(mode):
        for shift in range(16):
            _, view, _, _ = to_device(fr.body, shift)
            sets.append(cc.kernel_chunks(view.data_ptr() + fr.off[:-1], lens))
            decode_check(view, off, kv, ent)
    print(f"verifying decode ({mode}) on {cu_count()} CUs: " + cc.check_chunks(sets, cc.C, "one-entry blocks"))


@pytest.mark.parametrize("mode", MODES)
def test_verifying_decode_persistent_grid(mode):
    """(e): three blocks or more per wave of crc_kernel whatever its occupancy."""
    cus = cu_count()
    case = cc.persistent_kernel_case(cus)
    line = cc.check_persistent_kernel(len(case.blk_off) - 1, cus)
    rc, kv = O.decode_blocks(case.blocks, case.blk_off)
    assert rc == 0
    fr = case.framed()
    _, view, _, _ = to_device(fr.body, 3)
    with decode_mode(mode):
        decode_check(view, dev_off(fr.off), kv, np.arange(fr.nblk + 1))
    print(f"verifying decode ({mode}), persistent grid: " + line)


def flip_positions(fr, b):
    """{what: stream offset} of the bytes whose flip the checksum test must catch in block b."""
    s, L = int(fr.off[b]), int(fr.lens()[b])
    pos = {"first": s, "last": s + L - 1}
    for name, edges in (("stream", cc.stream_edges(L)), ("kernel", cc.kernel_edges(L))):
        pos[f"{name} edge - 1"], pos[f"{name} edge"] = s + edges[0] - 1, s + edges[0]
    for k in range(4):
        pos[f"crc byte {k}"] = s + L + k
    return pos


@pytest.mark.parametrize("mode", MODES)
def test_verifying_decode_catches_one_flipped_bit(mode):
    """One decode per flipped bit: a block's first and last byte, either side of its first chunk
    edge (the streaming kernel's and crc_kernel's), each stored CRC byte, in the batch's first,
    middle and last block -> LSMBLK_E_CHECKSUM.  A flip in the four bytes before the first block
    or after the last CRC is none of the decode's business."""
    case, fr, kv, ent = block_case()
    t, view, img, start = to_device(fr.body, 5)
    off = dev_off(fr.off)
    n = 0
    with decode_mode(mode):
        decode_check(view, off, kv, ent)
        for b in cc.victims(case):
            for what, p in flip_positions(fr, b).items():
                view[p] ^= 0x10
                st = decode_status(view, off)
                view[p] ^= 0x10
                assert st == LSMBLK_E_CHECKSUM, f"block {b}, {what}: status {st}"
                n += 1
        for p in list(range(start - 4, start)) + list(range(start + len(fr.body), start + len(fr.body) + 4)):
            t[p] ^= 0x10
            decode_check(view, off, kv, ent)
            t[p] ^= 0x10
        assert t.cpu().numpy().tobytes() == img.tobytes()
    print(f"verifying decode ({mode}): {n} flips caught in blocks {cc.victims(case)}, 8 outside ignored")


def recount(fr, b, count=b"\xff\xff"):
    """fr with block b's entry count overwritten and its stored CRC made right again."""
    body = fr.body.copy()
    e = int(fr.off[b + 1]) - 4
    body[e - 2:e] = np.frombuffer(count, np.uint8)
    body[e:e + 4] = np.frombuffer(zlib.crc32(body[int(fr.off[b]):e].tobytes()).to_bytes(4, "big"), np.uint8)
    return body


@pytest.mark.parametrize("mode", MODES)
def test_verifying_decode_reports_malformed_under_a_right_checksum(mode):
    """An entry count of 0xFFFF under a correct CRC, in a block of one chunk (counted from LDS in
    the two-pass mode) and in one of several (counted from global memory), and a framed range
    shorter than the tail -> LSMBLK_E_MALFORMED."""
    case, fr, _, _ = block_case()
    lens = case.lens()
    one = next(b for b in range(fr.nblk) if 1000 < lens[b] <= cc.C.kCrcChunk)
    many = cc.victims(case)[1]
    assert lens[many] > cc.C.kCrcChunk
    off = dev_off(fr.off)
    with decode_mode(mode):
        for b in (one, many):
            _, view, _, _ = to_device(recount(fr, b), 11)
            assert decode_status(view, off) == LSMBLK_E_MALFORMED, f"block {b} of {int(lens[b])} bytes"
        cut = int(fr.off[3])
        body = np.concatenate([fr.body[:cut], np.array([7, 9], np.uint8), fr.body[cut:int(fr.off[6])]])
        short = np.concatenate([fr.off[:4], fr.off[3:7] + 2])
        assert np.diff(short)[3] == 2
        _, view, _, _ = to_device(body, 2)
        assert decode_status(view, dev_off(short)) == LSMBLK_E_MALFORMED


# ------------------------------------------------------------------------------- f
def test_block_meta_section_crcs_at_every_shift():
    """(f): BlockMeta sections whose CRC'd region takes every length class, the section buffer at
    all 16 shifts: every section pyref's, its last four bytes zlib's CRC of the device's own
    section[4:-4], the bytes around the sections untouched."""
    case = cc.meta_case()
    want = cc.meta_sections(case)
    flat = np.frombuffer(b"".join(want), np.uint8)
    moff = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    nseg = len(want)
    _, blocks, _, _ = to_device(case.blocks, 0)
    boff = dev_off(case.blk_off.astype(np.int64))
    seg_blk = batch._u32_table(np.arange(nseg + 1, dtype=np.uint32), blocks.device)
    sets = []
    for shift in range(16):
        t, view, img, start = to_device(np.zeros(len(flat), np.uint8), shift, seed=1)
        sets.append(cc.kernel_chunks(*cc.meta_leads(case, view.data_ptr())))
        mo = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
        stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device="cuda")
        batch.block_meta_into(blocks, boff, nseg, seg_blk, nseg, view, len(flat), mo, stats)
        torch.cuda.synchronize()
        assert batch._status(stats) == 0 and int(stats[1]) == len(flat)
        assert mo.cpu().tolist() == moff.tolist()
        got = t.cpu().numpy()
        body = got[start:start + len(flat)]
        for s in np.flatnonzero([body[moff[s]:moff[s + 1]].tobytes() != want[s] for s in range(nseg)]):
            sec = body[moff[s]:moff[s + 1]].tobytes()
            what = "CRC" if sec[:-4] == want[s][:-4] else "bytes"
            pytest.fail(f"shift {shift}: {what} of section {s} ({case.region[s]} bytes under the CRC) differ")
        for s in range(nseg):
            sec = body[moff[s]:moff[s + 1]].tobytes()
            assert int.from_bytes(sec[-4:], "big") == zlib.crc32(sec[4:-4])
        assert got[:start].tobytes() == img[:start].tobytes() and got[start + len(flat):].tobytes() == img[start + len(flat):].tobytes()
    print("BlockMeta section CRCs: " + cc.check_chunks(sets, cc.C, "BlockMeta sections", section=True))
