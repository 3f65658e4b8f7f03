"""Batched SST point lookups on the device (lsmblk_sst_open_batch, lsmblk_sst_get_batch; lsm_amd.sst.SstSet)
against the CPU expectations of get_cases.py: what SsTable::open finds, every field of every lookup
in all four flag combinations at block_size 128 / 256 / 4096 and on both sides of kGetLdsBlock, the
gathered values, and the error reports."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import get_cases as gc
import gpu_kit as kit
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch, sst
from lsm_amd._lib import (LSMBLK_ERR_CAPACITY, LSMBLK_ERR_CHECKSUM, LSMBLK_ERR_EMPTY_KEY, LSMBLK_ERR_MALFORMED,
                          LSMBLK_ERR_SEGMENTS, LsmBlkError, SstIndexC)
from oracle import pyref

pytestmark = pytest.mark.gpu


def opened(name):
    return kit.opened_set(gc.case(name), ("get", name))


def img_ints(key):
    im = gc.image(key)
    return int.from_bytes(im[:8], "big"), int.from_bytes(im[8:], "big")


def check_open(ss, bufs):
    """Descriptors and index of every SST against pyref.sst_open of its bytes."""
    assert ss.open_stats[0] == len(bufs) and ss.open_stats[2] == 0 and ss.open_stats[3] == 0
    blk0 = 0
    for s, buf in enumerate(bufs):
        metas, max_ts, bloom, meta_offset = pyref.sst_open(buf)
        assert ss.err[s] == 0 and int(ss.desc["blk0"][s]) == blk0
        assert ss.num_of_blocks(s) == len(metas) and int(ss.desc["meta_offset"][s]) == meta_offset
        assert ss.first_key(s) == metas[0][1] and ss.last_key(s) == metas[-1][2]
        assert ss.max_ts(s) == max_ts and ss.bloom_k(s) == bloom.k and ss.bloom_filter(s) == bloom.filter
        offs = [m[0] for m in metas]
        assert ss.block_offsets(s).tolist() == offs + [meta_offset]
        assert ss.block_meta(s) == [(o, e, m[1]) for o, e, m in zip(offs, offs[1:] + [meta_offset], metas)]
        rec = ss.index[blk0:blk0 + len(metas)]
        assert [(int(r["img_hi"]), int(r["img_lo"])) for r in rec] == [img_ints(m[1]) for m in metas]
        blk0 += len(metas)
    assert ss.open_stats[1] == blk0


@pytest.mark.parametrize("name", gc.CASES)
def test_open_equals_pyref(name):
    check_open(opened(name), [s.buf for s in gc.case(name).ssts])


def test_open_of_files_written_on_the_device():
    """The same for files that lsmblk_sst_files_batch wrote, still in device memory."""
    c = gc.case("bs256")
    ents = [e for s in c.ssts for e in s.entries]
    keys = np.frombuffer(b"".join(k for k, _, _ in ents), np.uint8).copy()
    vals = np.frombuffer(b"".join(v for _, _, v in ents), np.uint8).copy()
    ko = np.concatenate([[0], np.cumsum([len(k) for k, _, _ in ents])]).astype(np.uint32)
    vo = np.concatenate([[0], np.cumsum([len(v) for _, _, v in ents])]).astype(np.uint32)
    kv = batch.KVStream.from_numpy(keys, ko, vals, vo, np.array([t for _, t, _ in ents], np.uint64))
    seg = np.concatenate([[0], np.cumsum([len(s.entries) for s in c.ssts])]).astype(np.uint32)
    r = batch.encode_sst(kv, seg, 256)
    files, off = sst.sst_files(r["blocks"], r["blk_off"], r["seg_blk"], seg, kv)
    ss = sst.SstSet(files, off)
    host, o = files.cpu().numpy().tobytes(), off.cpu().tolist()
    check_open(ss, [host[o[i]:o[i + 1]] for i in range(len(c.ssts))])
    exp, values, _ = gc.expected("bs256", False, False)
    got = ss.get(c.q_sst, c.keys, c.read_ts)
    assert (got["status"] == exp["status"]).all() and got["values"] == values


def corrupt(kind, buf):
    b = bytearray(buf)
    n = len(b)
    bo = int.from_bytes(b[n - 4:], "big")
    mo = int.from_bytes(b[bo - 4:bo], "big")
    if kind == "bloom-body":
        b[bo + 3] ^= 0x10
    elif kind == "meta-body":
        b[mo + 4 + 6] ^= 0x01          # a byte of the first block's first key
    elif kind == "bloom-offset-past-file":
        b[n - 4:] = struct.pack(">I", n + 100)
    elif kind == "meta-offset-past-bloom":
        b[bo - 4:bo] = struct.pack(">I", bo + 10)
    elif kind == "no-blocks":
        b[mo:mo + 4] = struct.pack(">I", 0)
    return bytes(b)


@pytest.mark.parametrize("kind,flag", [("bloom-body", LSMBLK_ERR_CHECKSUM), ("meta-body", LSMBLK_ERR_CHECKSUM),
                                       ("bloom-offset-past-file", LSMBLK_ERR_MALFORMED),
                                       ("meta-offset-past-bloom", LSMBLK_ERR_MALFORMED), ("no-blocks", LSMBLK_ERR_MALFORMED)])
def test_a_broken_sst_fails_alone(kind, flag):
    c = gc.case("bs256")
    bad = 1
    bufs = [corrupt(kind, s.buf) if i == bad else s.buf for i, s in enumerate(c.ssts)]
    ss = sst.SstSet(b"".join(bufs), c.file_off)
    assert ss.err.tolist() == [flag if i == bad else 0 for i in range(len(bufs))]
    assert ss.open_stats[0] == len(bufs) - 1 and ss.open_stats[2] == flag and ss.open_stats[3] == 0
    assert ss.num_of_blocks(bad) == 0
    exp, values, _ = gc.expected("bs256", False, False)
    got = ss.get(c.q_sst, c.keys, c.read_ts)
    other = np.array(c.q_sst) != bad
    for f in gc.FIELDS:
        assert (got[f][other] == exp[f][other]).all(), f
    assert [v for v, o in zip(got["values"], other) if o] == [v for v, o in zip(values, other) if o]
    # the failed SST answers ABSENT: an iterator over no blocks is invalid from the start
    assert (got["status"][~other] == gc.ABSENT).all() and (got["blk"][~other] == 0).all()
    assert (got["hit_blk"][~other] == gc.NONE).all()


@pytest.mark.parametrize("no_filter,mvcc", gc.MODES)
@pytest.mark.parametrize("name", gc.CASES)
def test_get_equals_expectation(name, no_filter, mvcc):
    c, ss = gc.case(name), opened(name)
    exp, values, val_off = gc.expected(name, no_filter, mvcc)
    got = ss.get(c.q_sst, c.keys, c.read_ts, no_filter=no_filter, mvcc=mvcc)
    for f in gc.FIELDS:
        bad = np.nonzero(got[f].astype(np.uint64) != exp[f])[0]
        assert not len(bad), (f, bad[:5], [c.keys[i] for i in bad[:5]], got[f][bad[:5]], exp[f][bad[:5]])
    assert got["val_off"].tolist() == val_off.tolist()
    assert got["values"] == values
    files = c.files
    for i in np.nonzero(got["status"] == gc.FOUND)[0]:  # val_pos / vlen point at the same bytes
        assert files[int(got["val_pos"][i]):int(got["val_pos"][i]) + int(got["vlen"][i])] == values[i]
    plain = ss.get(c.q_sst, c.keys, c.read_ts, no_filter=no_filter, mvcc=mvcc, values=False)
    assert "values" not in plain and all((plain[f] == got[f]).all() for f in gc.FIELDS)


@pytest.mark.parametrize("name,s", [("bs256", 0), ("bs128", 1), ("threshold", 0)])
def test_no_filter_landing_equals_find_block_idx_and_seek_batch(name, s):
    """(blk, ent) against the composition the library already had: host SsTable.find_block_idx,
    then lsmblk_seek_batch over the framed data section, then the spill."""
    c, ss = gc.case(name), opened(name)
    t = sst.SsTable(c.ssts[s].buf)
    sel = [i for i, x in enumerate(c.q_sst) if x == s]
    keys = [c.keys[i] for i in sel]
    qb = [t.find_block_idx(k) for k in keys]
    data = torch.frombuffer(bytearray(c.ssts[s].buf), dtype=torch.uint8).cuda()
    idx = batch.seek_blocks(data, torch.from_numpy(t.block_offsets().view(np.int64)).cuda(), qb, keys, tail=4)
    nent = [len(b) for b in c.ssts[s].blocks]
    want = [(b + 1, 0) if e == nent[b] else (b, int(e)) for b, e in zip(qb, idx)]
    got = ss.get(c.q_sst, c.keys, c.read_ts, no_filter=True, values=False)
    assert [(int(got["blk"][i]), int(got["ent"][i])) for i in sel] == want


def test_error_reports():
    c, ss = gc.case("threshold"), opened("threshold")
    keys, qs, ts = [b"a001", b"a002", b"b-at", b"a003"], [0, 7, 0, 0], [100, 100, 100, 100]
    r, _, _, st = ss.get_raw(qs, keys, ts)
    assert st[3] == LSMBLK_ERR_SEGMENTS and st[0] == 4
    assert r["status"].tolist() == [gc.FOUND, gc.ABSENT, gc.FOUND, gc.FOUND] and r["blk"][1] == gc.NONE
    with pytest.raises(LsmBlkError):
        ss.get(qs, keys, ts)
    r, _, _, st = ss.get_raw([0, 0, 0], [b"a001", b"", b"a003"], 100)
    assert st[3] == LSMBLK_ERR_EMPTY_KEY and r["status"].tolist() == [gc.FOUND, gc.ABSENT, gc.FOUND] and st[1] == 2
    # a too-small value buffer: CAPACITY, the required bytes, nothing written
    exp, values, val_off = gc.expected("threshold", False, False)
    need = int(val_off[-1])
    vals = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    r, _, vo, st = ss.get_raw(c.q_sst, c.keys, c.read_ts, val_cap=need - 1, vals=vals)
    assert st[3] == LSMBLK_ERR_CAPACITY and st[2] == need and (vals == 0xAB).all()
    assert (r["status"] == exp["status"]).all()
    r, _, vo, st = ss.get_raw(c.q_sst, c.keys, c.read_ts, val_cap=need, vals=vals)
    assert st[3] == 0 and st[2] == need and vo.tolist() == val_off.tolist() and st[1] == int((exp["status"] == gc.FOUND).sum())
    assert vals[:need].cpu().numpy().tobytes() == b"".join(v for v in values if v) and (vals[need:] == 0xAB).all()


def test_too_small_index_reports_the_required_count():
    c = gc.case("threshold")
    ss = sst.SstSet(c.files, c.file_off)
    total = sum(len(s.blocks) for s in c.ssts)
    assert len(ss.index) == total and ss.index_t.numel() >= total * ctypes.sizeof(SstIndexC)
    st = ss._open(total - 1)
    assert st[3] == LSMBLK_ERR_CAPACITY and st[1] == total and st[0] == 0
    st = ss._open(total)
    assert st[3] == 0 and st[0] == len(c.ssts)


def test_empty_batches():
    ss = opened("threshold")
    r, _, vo, st = ss.get_raw([], [], [], val_cap=16)
    assert st == [0, 0, 0, 0] and len(r) == 0 and vo.tolist() == [0]
    out = ss.get([], [], [])
    assert out["values"] == [] and len(out["status"]) == 0
    none = sst.SstSet(b"", [0])
    assert none.nsst == 0 and none.open_stats == [0, 0, 0, 0]
    assert none.get([], [], [])["values"] == []
    r, _, _, st = none.get_raw([0], [b"k"], 1)
    assert st[3] == LSMBLK_ERR_SEGMENTS and r["status"][0] == gc.ABSENT


# ------------------------------------------------------------------------------ the wrapper's retry
RETRY_BYTES = 3 * 2048  # the found values' bytes: more than the wrappers' first 64 * 4 + 1024


def capacity_retry_case():
    """(entries of one SST for block size 4096: 8 keys, one version each, 2048-byte values; 4 query
    keys, the third absent); test_gpu_lsm_get.py reads the same SST through a view."""
    ents = [(b"key%02d" % i, 5, bytes([65 + i]) * 2048) for i in range(8)]
    return ents, [ents[1][0], ents[4][0], b"key04x", ents[6][0]]


def check_capacity_retry(ss, raw, get, ents, keys, statuses):
    """get() -- ss.get or ss.lsm_get over the case -- calls ss.<raw> twice: CAPACITY with the bytes
    required, then every value."""
    seen, inner = [], getattr(ss, raw)

    def spy(*a, **kw):
        r = inner(*a, **kw)
        seen.append(r[3])
        return r

    setattr(ss, raw, spy)
    try:
        out = get()
    finally:
        delattr(ss, raw)
    assert [st[3] for st in seen] == [LSMBLK_ERR_CAPACITY, 0] and [st[2] for st in seen] == [RETRY_BYTES, RETRY_BYTES]
    by_key = {k: v for k, _, v in ents}
    assert out["status"].tolist() == statuses
    assert out["values"] == [by_key.get(k) for k in keys]
    assert int(out["val_off"][-1]) == RETRY_BYTES == 6144


def test_get_retries_once_on_capacity():
    """Found values of 6144 bytes against the wrapper's first buffer of 64 * 4 + 1024."""
    ents, keys = capacity_retry_case()
    s = gc.make_sst(ents, 4096)
    ss = sst.SstSet(s.buf, [0, len(s.buf)])
    statuses = [gc.lookup(s, k, 100, False, False)["status"] for k in keys]
    assert statuses.count(gc.FOUND) == 3
    check_capacity_retry(ss, "get_raw", lambda: ss.get([0] * 4, keys, 100), ents, keys, statuses)
