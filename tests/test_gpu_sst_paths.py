"""GPU parity of the SST container on the paths and thresholds no natural input reaches: device
fingerprint32 by key length with the key arena at every address residue, the bloom kernel on
both sides of its LDS switch and on its CRC chunk edges, sst_layout_kernel's rounds and carry,
meta_write_kernel's tile image on both sides of kMetaImg at every lead, the capacity contract of
lsmblk_sst_files_batch, and seek_kernel over long shared prefixes, prefix chains and whole blocks.

The inputs and their coverage conditions are tests/sst_cases.py's (checked on the CPU by
test_sst_cases.py); the address-dependent conditions are asserted again here for the tensors'
real addresses.  Every expected byte comes from oracle/ (pyref.sst_file, pyref.encode_block_meta,
O.seek_key over oracle-encoded blocks).
"""
import functools

import numpy as np
import pytest
import torch

import sst_cases as sc
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch
from lsm_amd import sst as S
from lsm_amd._lib import LSMBLK_E_CAPACITY
from oracle import oracle as O
from oracle import pyref
from test_gpu_parity import dev_blocks, to_dev
from test_gpu_paths import rehome

pytestmark = pytest.mark.gpu


def run_files(case, lay, d=None, nsst=None):
    """sst_files over the oracle's blocks of the first nsst SSTs -> (files u8 array, file_off list,
    files tensor address)."""
    d = d or to_dev(case.kv)
    nsst = len(case.ent) - 1 if nsst is None else nsst
    e, nb = sc.prefix(case, lay, nsst)
    if e < case.kv.n:  # a shorter stream: n entries, the key arena ends at key_off[n]
        d = batch.KVStream(d.keys[:int(case.kv.key_off[e])], d.key_off[:e + 1], d.vals, d.val_off[:e + 1], d.ts, e)
    db, do = dev_blocks(lay.blocks[:int(lay.blk_off[nb])], lay.blk_off[:nb + 1])
    files, off = S.sst_files(db, do, lay.sst_blk[:nsst + 1], case.ent[:nsst + 1], d)
    return files.cpu().numpy(), off.cpu().tolist(), files.data_ptr()


def files_check(got, off, want, case, lay, what=""):
    """file_off == the running sum of the expected lengths and every file == its expectation; a
    mismatch names the first differing SST, its first key's length and the section."""
    lens = [len(w) for w in want]
    n = len(want)
    # the classifier's layout is the oracle's: lengths and both footers
    assert lens == lay.file_len[:n].tolist(), f"{what}: layout() against pyref"
    assert [int.from_bytes(w[-4:], "big") for w in want] == lay.bloom_off[:n].tolist()
    assert [int.from_bytes(w[int(o) - 4:int(o)], "big") for w, o in zip(want, lay.bloom_off)] == lay.data_len[:n].tolist()
    assert off == np.concatenate([[0], np.cumsum(lens)]).tolist(), f"{what}: file_off"
    flat = np.frombuffer(b"".join(want), np.uint8)
    assert len(got) == len(flat), what
    mism = np.flatnonzero(got != flat)
    if mism.size:
        s = int(np.searchsorted(off, mism[0], side="right")) - 1
        e = int(case.ent[s])
        kl = int(case.kv.key_off[e + 1] - case.kv.key_off[e])
        byte = int(mism[0]) - off[s]
        pytest.fail(f"{what}: SST {s} (first key {kl} B, {int(case.ent[s + 1]) - e} entries) differs in its "
                    f"{sc.section_of(lay, s, byte)} section at byte {byte} of {lens[s]}; {mism.size} bytes differ in all")


# ------------------------------------------------------------------------------- 1. fingerprint32
@functools.lru_cache(None)
def _fp_base():
    case = sc.fingerprint_stream()
    sc.check_fingerprint_stream(case)
    return case, sc.expected_files(case)


@pytest.mark.parametrize("cls", range(4), ids=sc.FP_CLASSES)
def test_device_fingerprint32_by_key_length(cls):
    """265 one-entry SSTs (one key per 64-bit filter), key lengths 1..130 plain and with every byte
    >= 0x80, then 200..1000; the stream's last key of length class `cls`; the key arena at every
    address residue mod 16."""
    base, base_want = _fp_base()
    last = sc.fp_last_indices(base)[cls]
    case, perm = sc.reorder_last(base, last)
    want = [base_want[i] for i in perm]
    assert want[-1] == pyref.sst_file([case.kv.entry(case.kv.n - 1)], 16)
    lay = sc.layout(case)
    seen = set()
    for shift in range(16):
        d = to_dev(case.kv)
        d.keys = rehome(d.keys, shift)
        seen.add(d.keys.data_ptr() % 16)
        got, off, _ = run_files(case, lay, d)
        files_check(got, off, want, case, lay, f"key arena at {shift} mod 16, last key {case.tag[-1]} B")
    assert seen == set(range(16))
    cnt = np.bincount(sc.fp_class(case.tag), minlength=4)
    print(f"fingerprint32: {len(case.tag)} keys, classes {dict(zip(sc.FP_CLASSES, cnt.tolist()))}, loop counts "
          f"{sorted(set(sc.fp_iters(np.asarray(case.tag)[np.asarray(case.tag) > 24]).tolist()))}, last key "
          f"{case.tag[-1]} B ({sc.FP_CLASSES[cls]}), arena residues {sorted(seen)}, block lengths mod 16 "
          f"{sorted(set((np.diff(lay.blk_off.astype(np.int64)) % 16).tolist()))}")


# ------------------------------------------------------------------------------- 2. bloom
@pytest.mark.parametrize("group", ["min", "lds-a", "lds-b", "global"])
def test_bloom_filter_size_and_path(group):
    """SSTs whose nbytes + 1 sits on the LDS switch, on crc_lds's chunk edges (1, 2, 3 chunks), on
    the global fold's chunk edges and on the 64-bit floor; the global-path SSTs in one call, each
    after a filler that steers its bloom address through the four values of address & 3."""
    case = sc.bloom_stream(group)
    lay = sc.layout(case)
    want = sc.expected_files(case)
    got, off, addr = run_files(case, lay)
    files_check(got, off, want, case, lay, group)
    assert addr % 16 == 0
    real = [s for s, n in enumerate(case.tag) if n]
    paths = [(case.tag[s],) + sc.bloom_path(case.tag[s]) for s in real]
    dsh = sorted({int(addr + sc.bloom_addr(lay, s)) & 3 for s in real})
    if group == "global":
        assert sc.check_bloom_global(case, lay, addr) == [0, 1, 2, 3]
    else:
        assert all(p[1] == "lds" for p in paths)
    print(f"bloom {group}: (keys, path, CRC chunks) {paths}; nbytes+1 {[int(lay.bloom_len[s]) for s in real]}; "
          f"bloom address & 3 {dsh}")


# ------------------------------------------------------------------------------- 3. layout
@functools.lru_cache(None)
def _layout_base():
    case = sc.layout_stream()
    lay = sc.layout(case)
    sc.check_layout_stream(case, lay)
    return case, lay, sc.expected_files(case)


@pytest.mark.parametrize("nsst", sc.LAYOUT_NSST)
def test_file_layout_over_many_ssts(nsst):
    """sst_layout_kernel's rounds of 1024 SSTs and their carry, sst_of_block over thousands of SSTs:
    one-entry and two-entry SSTs, file_off and every file against pyref."""
    case, lay, want = _layout_base()
    got, off, _ = run_files(case, lay, nsst=nsst)
    files_check(got, off, want[:nsst], case, lay, f"{nsst} SSTs")
    print(f"layout: {nsst} SSTs = {-(-nsst // sc.LAYOUT_ROUND)} rounds of {sc.LAYOUT_ROUND}, "
          f"{(nsst - 1) % sc.LAYOUT_ROUND + 1} in the last; {sc.prefix(case, lay, nsst)[1]} blocks, {off[-1]} bytes")


# ------------------------------------------------------------------------------- 4. BlockMeta tiles
PATTERN = 251


def sentinel(n):
    return (torch.arange(n, device="cuda") % PATTERN).to(torch.uint8)


def meta_check(case, seg_blk, lay, meta, shift, what):
    """block_meta_into with the section buffer at meta[64 + shift:]: offsets and bytes against
    pyref, the bytes around the sections untouched."""
    want = sc.expected_metas(case, seg_blk)
    flat = np.frombuffer(b"".join(want), np.uint8)
    nseg, nblk = len(seg_blk) - 1, len(lay.blk_off) - 1
    assert meta.numel() >= 64 + shift + len(flat) + 64
    meta.copy_(sentinel(meta.numel()))
    db, do = dev_blocks(lay.blocks, lay.blk_off)
    view = meta[64 + shift:64 + shift + len(flat)]
    moff = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
    stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device="cuda")
    batch.block_meta_into(db, do, nblk, batch._u32_table(seg_blk, db.device), nseg, view, len(flat), moff, stats)
    torch.cuda.synchronize()
    assert batch._status(stats) == 0 and int(stats[1]) == len(flat), what
    assert moff.cpu().tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist(), what
    got = meta.cpu().numpy()
    body = got[64 + shift:64 + shift + len(flat)]
    mism = np.flatnonzero(body != flat)
    if mism.size:
        g = int(np.searchsorted(moff.cpu().numpy(), mism[0], side="right")) - 1
        pytest.fail(f"{what}: section {g} differs at byte {int(mism[0])} of {len(flat)}; {mism.size} bytes in all")
    guard = sentinel(meta.numel()).cpu().numpy()
    assert np.array_equal(got[:64 + shift], guard[:64 + shift]), f"{what}: bytes before the sections changed"
    end = 64 + shift + len(flat)
    assert np.array_equal(got[end:], guard[end:]), f"{what}: bytes after the sections changed"


@pytest.mark.parametrize("shift", [0, 5])
def test_block_meta_tile_image_edges(shift):
    """46 tiles of kMetaTile blocks whose lead + span takes every value in kMetaImg +- 8 (kMetaImg
    and kMetaImg + 1 at four leads each), every lead and span & 15 on the LDS side; segment
    boundaries on, before and after a tile edge, empty segments, a last tile of one block -- the
    section buffer at two address residues; then the first kMetaTile - 1, kMetaTile and
    kMetaTile + 1 blocks alone."""
    meta = torch.zeros(2 << 20, dtype=torch.uint8, device="cuda")
    assert meta.data_ptr() % 16 == 0
    addr = meta.data_ptr() + 64 + shift
    case, seg_blk = sc.meta_stream(addr)
    lay = sc.layout(case)
    t = sc.check_meta_stream(case, seg_blk, lay, addr)
    meta_check(case, seg_blk, lay, meta, shift, f"meta at {addr % 16} mod 16")
    print(sc.meta_coverage(f"meta at {addr % 16} mod 16", t))
    cnt = sc.pc.block_entry_counts(lay.blocks, lay.blk_off.astype(np.int64))
    for nb in (sc.C.kMetaTile - 1, sc.C.kMetaTile, sc.C.kMetaTile + 1):
        e = int(cnt[:nb].sum())
        kv = case.kv
        sub = sc.Case(O.KV(kv.keys[:int(kv.key_off[e])], kv.key_off[:e + 1], kv.vals[:int(kv.val_off[e])],
                           kv.val_off[:e + 1], kv.ts[:e]), np.array([0, e], np.uint32), case.bs)
        sl = sc.layout(sub)
        assert len(sl.blk_off) - 1 == nb
        meta_check(sub, np.array([0, nb], np.uint32), sl, meta, shift, f"{nb} blocks")


def test_block_meta_tiles_through_sst_files():
    """The same tiles (no empty SSTs) through lsmblk_sst_files_batch, whose meta sections are
    composed in the context's workspace (256-byte aligned)."""
    case, seg_blk = sc.meta_stream(0, empty_segments=False)
    lay = sc.layout(case)
    t = sc.check_meta_stream(case, seg_blk, lay, 0)
    assert np.array_equal(seg_blk, lay.sst_blk)
    got, off, _ = run_files(case, lay)
    files_check(got, off, sc.expected_files(case), case, lay, "tile stream")
    print(sc.meta_coverage("meta in the workspace", t))


# ------------------------------------------------------------------------------- 5. capacity
@pytest.mark.parametrize("which", ["layout", "global"])
def test_sst_files_capacity_contract(which):
    """stats[1] = the bytes required; one byte short: CAPACITY and nothing written; exactly enough:
    success and not a byte outside; no buffer at all: CAPACITY and the size."""
    case = sc.capacity_stream(which)
    lay = sc.layout(case)
    assert lay.file_off[1] & 3 == 1
    want = np.frombuffer(b"".join(sc.expected_files(case)), np.uint8)
    total, nsst, nblk = len(want), len(case.ent) - 1, len(lay.blk_off) - 1
    assert total == lay.file_off[-1]
    d = to_dev(case.kv)
    db, do = dev_blocks(lay.blocks, lay.blk_off)
    sb, se = batch._u32_table(lay.sst_blk, db.device), batch._u32_table(case.ent, db.device)
    foff = torch.zeros(nsst + 1, dtype=torch.int64, device="cuda")
    stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device="cuda")
    buf = torch.zeros(total + 128, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    guard = sentinel(buf.numel())

    def call(files, cap):
        buf.copy_(guard)
        S.sst_files_into(db, do, nblk, sb, se, nsst, d, files, cap, foff, stats)
        torch.cuda.synchronize()
        return batch._status(stats), int(stats[1])

    assert call(buf[64:64 + total - 1], total - 1) == (LSMBLK_E_CAPACITY, total)
    assert torch.equal(buf, guard), "CAPACITY, yet bytes were written"
    assert call(None, 0) == (LSMBLK_E_CAPACITY, total)
    assert call(buf[64:64 + total], total) == (0, total)
    got = buf.cpu().numpy()
    files_check(got[64:64 + total], foff.cpu().tolist(), sc.expected_files(case), case, lay, which)
    g = guard.cpu().numpy()
    assert np.array_equal(got[:64], g[:64]), "bytes before the buffer changed"
    assert np.array_equal(got[64 + total:], g[64 + total:]), "bytes after the buffer changed"
    print(f"capacity {which}: {nsst} SSTs, {total} bytes, first real file at {int(lay.file_off[1])} "
          f"({int(lay.file_off[1]) & 3} mod 4), bloom paths {sorted({sc.bloom_path(int(n))[0] for n in np.diff(case.ent.astype(np.int64))})}")


# ------------------------------------------------------------------------------- 6. seek
def seek_check(c, tail=0):
    want = c.expected()
    assert all(w == s for w, s in zip(want, c.q_self) if s >= 0), "the oracle misses an entry's own key"
    blocks, off = c.blocks, c.blk_off
    if tail:
        framed = b"".join(c.block(b) + O.crc32(c.block(b)).to_bytes(4, "big") for b in range(len(off) - 1))
        blocks = np.frombuffer(framed, np.uint8).copy()
        off = np.concatenate([[0], np.cumsum(np.diff(off.astype(np.int64)) + 4)]).astype(np.uint64)
    db, do = dev_blocks(blocks, off)
    got = batch.seek_blocks(db, do, c.q_blk, c.q_key, tail=tail).tolist()
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (f"{len(bad)} of {len(want)} probes; first: block {c.q_blk[bad[0]]}, key {c.q_key[bad[0]].hex()}, "
                     f"got {got[bad[0]]}, want {want[bad[0]]}")


@pytest.mark.parametrize("name", ["prefix-1024", "prefix-4096", "chain-256", "chain-4096", "big", "tiny"])
def test_seek_prefixes_chains_and_whole_blocks(name):
    """seek_kernel against O.seek_key: keys that share 20-60 bytes with their block's first key,
    chains of keys that are prefixes of one another, every entry of whole blocks (one of 64 KiB
    with over 2000 entries) probed with its key, key + 0x00, key minus a byte and its neighbours,
    the empty probe and 300 bytes of 0xFF, one-entry and two-entry blocks; "prefix-1024" and "tiny"
    also in the framed layout."""
    kind, _, bs = name.partition("-")
    c = {"prefix": lambda: sc.seek_prefix_case(int(bs)), "chain": lambda: sc.seek_chain_case(int(bs)),
         "big": sc.seek_big_case, "tiny": sc.seek_tiny_case}[kind]()
    if kind == "prefix":
        p = c.prefix_lens()
        assert 0 in p and 1 in p and len(set(p[p >= 20].tolist())) >= 40
    if kind == "big":
        assert int.from_bytes(c.block(0)[-2:], "big") > 2000
    seek_check(c)
    if name in ("prefix-1024", "tiny"):
        seek_check(c, tail=4)
    print(sc.seek_coverage("seek " + name, c))
