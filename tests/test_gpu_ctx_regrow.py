"""A context's workspaces across calls of different sizes: small -> large -> small on one context.

Every context buffer (DevBuf, lsmblk_dev.hpp) grows to need + need / 4 + 1024 elements when a call
needs more than it holds, so a context that served a small call has to free, reallocate and zero
its buffers -- on the call's stream, and for the uncached status arrays with a new epoch sequence
-- when a large one follows, and the small call after that runs in the large call's buffers.  Each
sequence below runs on a fresh torch.cuda.Stream, which gives it a fresh context, and every call's
output is compared with the expectation the family's own GPU test uses (the C oracle, oracle/pyref.py
or the closed forms of the *_cases.py modules).

  small   8 entries, one segment / run pair / SST, 2 blocks (block_size 128)
  large   4096 entries at block_size 64: 2048 blocks, and 2048 segments / SSTs / ranges where the
          call takes them

The per-family comments state why the large call's need exceeds the capacity the small call left
(need + need / 4 + 1024).  The per-tile buffers (one element per 64 blocks or per 1024 entries) are
the exception: a small call leaves room for 1025 tiles, which only a batch of > 65 000 blocks passes;
they are reused, not regrown, here.
"""
import contextlib
import zlib
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import get_cases as gc
import lsm_get_cases as lc
import lsm_scan_cases as ls
import merge_newest_cases as mn
import scan_cases as sc
from gpu_kit import _need_gpu, check_stream  # noqa: F401 (_need_gpu: autouse)
from lsm_amd import batch, shard, sst
from lsm_amd._lib import (LSMBLK_DEBUG_SCAN_UNITS, LSMBLK_MERGE_NEWEST, LSMBLK_MERGE_RUNS, LSMBLK_MERGE_TWO_LEVEL, lib)
from oracle import oracle as O
from oracle import pyref
from test_gpu_compact import assert_kv_equal, check_compact, dev_entries, to_dev
from test_gpu_crc_paths import decode_mode
from test_gpu_get import check_open
from test_gpu_parity import _meta_check, dev_blocks, framed_check, framed_want, slot_check
from test_gpu_shard import check_against_single_stream

pytestmark = pytest.mark.gpu

N = {"small": 8, "large": 4096}
BS = {"small": 128, "large": 64}
SML = ("small", "large", "small")
SCAN_UNITS = 64  # the scans' unit budget here (default 2^17 units = 3 MiB, which no small batch outgrows)
TS_MAX = (1 << 64) - 1


@contextlib.contextmanager
def fresh_context():
    """A stream no call has used made current: the wrappers' default stream, hence a fresh context.
    torch hands out its streams from a pool of 32, so a stream that an earlier test has left a
    context on is passed over, and the sequence releases its own context when it is done.  (Only its
    own: the other modules' contexts hold GiB of workspace, and tearing those down in the middle of
    the suite is not what this test is about.)"""
    dev = torch.cuda.current_device()
    for _ in range(64):
        s = torch.cuda.Stream()
        if (dev, s.cuda_stream) not in batch._ctxs:
            break
    else:
        pytest.fail("every stream of the pool already has a context")
    try:
        with torch.cuda.stream(s):
            yield s
    finally:
        s.synchronize()
        batch.release_contexts(dev, s)


def run_sequence(step, sizes=SML):
    with fresh_context():
        for size in sizes:
            step(size)


# ---------------------------------------------------------------- the two inputs, built once
def entry(i, ts=1):
    return (b"key%05d" % i, ts, b"v%03d" % (i % 1000))  # 8-byte key, 4-byte value


@lru_cache(maxsize=None)
def stream_of(size):
    """(kv, segments, oracle blocks, oracle offsets, oracle decode): one segment (small), 2048 (large)."""
    n = N[size]
    kv = O.KV.from_entries([entry(i) for i in range(n)])
    seg = np.array([0, n], np.uint32) if size == "small" else np.arange(0, n + 1, 2, dtype=np.uint32)
    rc, blocks, off = O.encode_segments(kv, seg, BS[size])
    assert rc == 0
    # a first entry takes 26 + 2 bytes and a later one of the same prefix 19 + 2: five fit a 128-byte
    # block and two a 64-byte one
    assert len(off) - 1 == (2 if size == "small" else 2048)
    rc, dec = O.decode_blocks(blocks, off)
    assert rc == 0
    return kv, seg, blocks, off, dec


@lru_cache(maxsize=None)
def runs_of(size):
    """A run pair of n entries: the newer run over keys [0, n/2), the older over [n/4, 3n/4)."""
    n = N[size]
    runs = [[entry(i, 2) for i in range(n // 2)], [entry(i, 1) for i in range(n // 4, 3 * n // 4)]]
    kv = O.KV.from_entries([e for r in runs for e in r])
    return runs, kv, np.array([0, n // 2, n], np.uint32)


@lru_cache(maxsize=None)
def versions_of(size):
    """n entries in merged order: n/2 keys, two versions each, every third older one a tombstone."""
    ents = []
    for i in range(N[size] // 2):
        k, _, v = entry(i)
        ents += [(k, 2, v), (k, 1, b"" if i % 3 == 0 else v + b"-old")]
    return ents


@lru_cache(maxsize=None)
def tables_of(size):
    """The stream as SST files: one of 8 entries (small), 2048 of 2 entries each (large)."""
    n, per = N[size], (8 if size == "small" else 2)
    ents = [entry(i) for i in range(n)]
    ssts = [gc.make_sst(ents[i:i + per], BS[size]) for i in range(0, n, per)]
    assert sum(len(s.blocks) for s in ssts) == (2 if size == "small" else 2048)
    # the small view has its table in L0, the large one all 2048 in one level
    l0, levels = ([0], []) if size == "small" else ([], [list(range(len(ssts)))])
    return lc.View(size, ssts, l0, levels, [], [])


def opened(size):
    v = tables_of(size)
    ss = sst.SstSet(v.files, v.file_off)
    return v, ss, ss.view(v.l0, v.levels)


def few(v, k=64):
    """Up to k tables of the view, spread over it."""
    return list(range(0, len(v.ssts), max(1, len(v.ssts) // k)))[:k]


# ---------------------------------------------------------------- decode
# dec_agg: 3 words per block, the small call leaves room for 2 + 0 + 1024 = 1026 blocks < 2048.
# lag_gran (status memory, lagged decode): covers blocks + blocks / 4 + 1024 = 1026 blocks < 2048, so
# the large call synchronizes, frees and reallocates it and restarts the epochs.  vcrc (verifying
# decode): nblk + 1 = 3 -> 1027 < 2049.  tile_sum / tile_pre: 1 tile -> 1025 >= 32, reused.
@pytest.mark.parametrize("verify", (False, True))
@pytest.mark.parametrize("mode", ("lagged", "two_pass"))
def test_decode(mode, verify):
    def step(size):
        kv, seg, blocks, off, dec = stream_of(size)
        with decode_mode(mode):
            if verify:
                want, want_off = framed_want(blocks, off)
                db, do = dev_blocks(np.frombuffer(want, np.uint8).copy(), want_off)
                got = batch.decode_blocks(db, do, tail=4, verify=True)
            else:
                got = batch.decode_blocks(*dev_blocks(blocks, off))
        assert_kv_equal(got, dec)
    run_sequence(step)


# ---------------------------------------------------------------- encode
# rec_first / blk_first / ent / big_list / blk_sz: n + 1 = 9 entries -> room for 9 + 2 + 1024 = 1035
# < 4097.  seg_agg / seg_inc (status memory): 1 segment -> 1025 < 2048: reallocated, epoch reset.
# The fused launch's frec: n + walkers + 1 = 13 records -> 1040 < 4096 + 512 + 1; fbig likewise;
# fdone / fwnb: 4 walkers -> 1029 >= 512, reused.  The fourth and fifth small calls go on counting
# epochs in the arrays the large call allocated.
def test_encode_packed_slots_framed_and_fused():
    def step(size):
        kv, seg, blocks, off, _ = stream_of(size)
        got, got_off = batch.encode_kv(to_dev(kv), seg, BS[size])
        np.testing.assert_array_equal(got_off.cpu().numpy().view(np.uint64), off)
        np.testing.assert_array_equal(got.cpu().numpy(), blocks)
        slot_check(kv, seg, BS[size], blocks, off)    # slots, and slots through the fused launch
        framed_check(kv, seg, BS[size], blocks, off)  # framed packed (read back verifying), framed slots
    run_sequence(step, SML + ("small", "small"))


# ---------------------------------------------------------------- CRC
# lsmblk_crc32_batch holds no buffer that depends on the batch (the tables are allocated once, by
# the first call): the sequence checks that the one allocation serves every size.
def test_crc32():
    def step(size):
        _, _, blocks, off, _ = stream_of(size)
        got = batch.crc32_blocks(*dev_blocks(blocks, off)).cpu().numpy().view(np.uint32)
        want = [zlib.crc32(bytes(blocks[int(a):int(b)])) for a, b in zip(off[:-1], off[1:])]
        np.testing.assert_array_equal(got, np.array(want, np.uint32))
    run_sequence(step)


# ---------------------------------------------------------------- BlockMeta sections
# meta_rec / meta_pos: nblk + 1 = 3 -> 1027 < 2049.  meta_crc: 1 segment -> 1025 < 2048.
# meta_tile: tiles + 1 -> 1026, reused.  (encode_sst also runs the encode, the segment table and the
# CRC pass on the same context.)
def test_block_meta():
    def step(size):
        kv, seg, _, _, _ = stream_of(size)
        _meta_check(kv, seg, BS[size])
    run_sequence(step)


# ---------------------------------------------------------------- the two filters
# filt_keep: n + 1 = 9 -> 1035 < 4097.  filt_tile: tiles + 1 = 2 -> 1026, reused.
def test_compact_filter_and_read_filter():
    def step(size):
        ents = versions_of(size)
        d = to_dev(O.KV.from_entries(ents))
        got = batch.compact_filter(d, 1, True)
        assert_kv_equal(got, O.KV.from_entries(pyref.compact_filter_loop(ents, 1, True, ())))
        seg = [0, len(ents)] if size == "small" else list(range(0, len(ents) + 1, 2))
        rows = [sc.read_filter_rule(ents[a:b], 1) for a, b in zip(seg[:-1], seg[1:])]
        got, got_seg = batch.read_filter(d, np.array(seg, np.uint32), 1)
        assert_kv_equal(got, O.KV.from_entries([e for r in rows for e in r]))
        assert got_seg.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in rows])]).tolist()
    run_sequence(step)


# ---------------------------------------------------------------- merge
# cws, one arena in bytes: the plan of an 8-entry merge is 21 regions of <= 256 bytes (about 5.5 KiB,
# which leaves about 8 KiB); the 4096-entry plan's k16 region alone is 16 * 4097 bytes.
def merge_want(size, mode):
    runs, kv, rs = runs_of(size)
    if mode == LSMBLK_MERGE_TWO_LEVEL:
        return pyref.two_merge_runs(runs)
    if mode == LSMBLK_MERGE_NEWEST:
        return O.gather(kv, mn.newest_order(SimpleNamespace(runs=lambda: runs, rs=rs))).entries()
    return O.gather(kv, O.merge_runs(kv, rs)).entries()


def merge_step(size, mode=LSMBLK_MERGE_RUNS):
    _, kv, rs = runs_of(size)
    assert dev_entries(batch.merge_runs(to_dev(kv), rs, merge_mode=mode)) == merge_want(size, mode)


@pytest.mark.parametrize("mode", (LSMBLK_MERGE_RUNS, LSMBLK_MERGE_TWO_LEVEL, LSMBLK_MERGE_NEWEST))
def test_merge(mode):
    run_sequence(lambda size: merge_step(size, mode))


# ---------------------------------------------------------------- SST rotation
# cws: the rotation plan of 9 slots is 8 regions of 256 bytes; of 4097 slots, rec alone 16 KiB.
def rotation_step(size):
    kv = stream_of(size)[0]
    np.testing.assert_array_equal(batch.sst_rotation(to_dev(kv), BS[size], 256),
                                  O.segment_like_compaction(kv, BS[size], 256))


def test_sst_rotation():
    run_sequence(rotation_step)


# ---------------------------------------------------------------- fused compaction
# cws holds the merge plan, the rotation plan and the stage stats (as above, KiB against hundreds of
# KiB); the encode's buffers as in the encode family; the rotation runs on the context's second
# stream, forked and joined in every call.
def compact_step(size):
    _, kv, rs = runs_of(size)
    check_compact(kv, rs, 0, False, (), BS[size], 256)


def test_compact_batch():
    run_sequence(compact_step)


# ---------------------------------------------------------------- merge + rules of one key range
# cws as in the merge family.
def test_compact_merge():
    def step(size):
        _, kv, rs = runs_of(size)
        src = O.merge_runs(kv, rs)
        want = O.compact(kv, src, 1, True, (), BS[size], 256)
        d = to_dev(kv)
        kb, vb = d.byte_sizes()
        kept = batch.KVStream.empty(d.n, kb, vb, torch.device("cuda"))
        stats = torch.zeros(5, dtype=torch.int64, device="cuda")
        opts = batch.compact_opts(1, True, (), BS[size], 256)
        batch.compact_merge_into(d, batch._u32_table(rs, "cuda"), 2, opts, None, kept, stats)
        torch.cuda.synchronize()
        s = stats.cpu().tolist()
        ref = O.gather(kv, src[want["kept"]])
        assert s == [ref.n, int(ref.key_off[-1]), int(ref.val_off[-1]), 0, len(src)]
        kept.n = s[0]
        assert_kv_equal(kept, ref)
    run_sequence(step)


# ---------------------------------------------------------------- key-range shard: prepare, carry, encode
# One context (an OwnCtx) for three shards in turn.  rws: the shard rotation plan of 9 slots is a
# few KiB, of 4097 slots hundreds; cws (the shard's merge) and the encode's buffers as above.
def test_shard_calls():
    ctx = None

    def step(size):
        nonlocal ctx
        _, kv, rs = runs_of(size)
        opts = batch.compact_opts(1, True, (), BS[size], 256)
        sh = shard.RangeShard(to_dev(kv), rs, opts)
        ctx = ctx or sh.ctx
        sh.ctx = ctx  # the one context of the sequence
        check_against_single_stream(kv, rs, shard.compact_local([sh]), 1, True, BS[size], 256)
    run_sequence(step)


# ---------------------------------------------------------------- SST files
# sws: block CRCs 4 * (nblk + 1), two tables of 8 * (nsst + 1), the BlockMeta sections: five regions
# of 256 bytes for the small call, 8 KiB + 2 * 16 KiB + > 100 KiB for the large one.
def files_step(size):
    v = tables_of(size)
    ents = [e for s in v.ssts for e in s.entries]
    kv = to_dev(O.KV.from_entries(ents))
    seg = np.concatenate([[0], np.cumsum([len(s.entries) for s in v.ssts])]).astype(np.uint32)
    r = batch.encode_sst(kv, seg, BS[size])
    files, off = sst.sst_files(r["blocks"], r["blk_off"], r["seg_blk"], seg, kv)
    assert off.cpu().tolist() == v.file_off
    assert files.cpu().numpy().tobytes() == v.files


def test_sst_files():
    run_sequence(files_step)


# ---------------------------------------------------------------- open + point reads
# sws (the open): 8 * (4 nsst + 1) + 16 nsst + 256 bytes, three regions of 256 for one SST (room for
# 1984 bytes) against 64 KiB + 32 KiB for 2048.  The point read itself holds no workspace.
def open_step(size):
    v, ss, _ = opened(size)
    check_open(ss, [s.buf for s in v.ssts])
    return v, ss


def test_sst_open_and_get():
    def step(size):
        v, ss = open_step(size)
        q_sst, keys = [], []
        for t in few(v):
            first = v.ssts[t].entries[0][0]
            q_sst += [t, t, t]
            keys += [first, first + b"x", v.ssts[t].entries[-1][0]]
        read_ts = [5, 5, 0] * (len(keys) // 3)
        rows = [gc.lookup(v.ssts[t], k, ts, False, False) for t, k, ts in zip(q_sst, keys, read_ts)]
        got = ss.get(q_sst, keys, read_ts)
        for f in gc.FIELDS:
            want = [(0 if r[f] is None else v.file_off[t] + r[f]) if f == "val_pos" else r[f] for r, t in zip(rows, q_sst)]
            assert got[f].astype(np.uint64).tolist() == want, f
        assert got["values"] == [r["value"] for r in rows]
    run_sequence(step)


# ---------------------------------------------------------------- point reads over a view
# sws: 256 bytes whatever the batch; the large call follows the large open (above) on its context.
def lsm_get_step(size):
    v, ss, view = opened(size)
    keys = [k for t in few(v) for k in (v.ssts[t].entries[0][0], v.ssts[t].entries[0][0] + b"x")]
    read_ts = [5, 0] * (len(keys) // 2)
    exp, values, _ = lc.arrays(v, [lc.closed(v, k, ts, "default") for k, ts in zip(keys, read_ts)])
    got = ss.lsm_get(view, keys, read_ts)
    for f in lc.FIELDS:
        assert got[f].astype(np.uint64).tolist() == exp[f].tolist(), f
    assert got["values"] == values


def test_lsm_get():
    run_sequence(lsm_get_step)


# ---------------------------------------------------------------- range scans
@contextlib.contextmanager
def scan_units():
    h = batch._ctx(torch.cuda.current_device())
    assert lib().lsmblk_debug_set(h, LSMBLK_DEBUG_SCAN_UNITS, SCAN_UNITS) == 0
    try:
        yield
    finally:
        assert lib().lsmblk_debug_set(h, LSMBLK_DEBUG_SCAN_UNITS, 0) == 0


def table_ranges(v, nq):
    """nq ranges, range i the whole of table i mod 64 by its first and last key (both included)."""
    pick = few(v)
    t = [pick[i % len(pick)] for i in range(nq)]
    return t, [v.ssts[x].entries[0][0] for x in t], [v.ssts[x].entries[-1][0] for x in t]


# sws, with a budget of 64 units: ubase 4 (nq + 1), qbad 4 nq, hdr 256, ucnt 24 (nq + 64) bytes: one
# range takes 2560 bytes (room for 4224), 2048 ranges 8 KiB + 8 KiB + 256 + 50 KiB.
def scan_step(size):
    v, ss, _ = opened(size)
    nq = 1 if size == "small" else 2048
    q_sst, lower, upper = table_ranges(v, nq)
    rows = [sc.scan_one(v.ssts[t], sc.INCLUDED, lo, sc.INCLUDED, up, False, False) for t, lo, up in zip(q_sst, lower, upper)]
    ents = [r["entries"] for r in rows]
    caps = (sum(len(e) for e in ents), sum(len(k) for e in ents for k, _, _ in e), sum(len(x) for e in ents for _, _, x in e))
    with scan_units():
        r, seg, kv, st = ss.scan_raw(q_sst, lower, upper, [sc.INCLUDED] * nq, [sc.INCLUDED] * nq, 0, caps)
    assert st == [*caps, 0]
    for f in sc.FIELDS:
        assert r[f].astype(np.uint64).tolist() == [row[f] for row in rows], f
    check_stream(kv, ents, seg)


def test_sst_scan():
    run_sequence(scan_step)


# sws, with a budget of 64 units and sub_cap = nq table scans: 14 regions of 256 bytes and 24 * 65
# for one range (about 5 KiB, room for about 7 KiB); for 2048 ranges the table scans' results alone
# are 32 * 2048 bytes.  head, pbad and mcnt are zeroed by every call, the slots too.
def lsm_scan_step(size):
    v, ss, view = opened(size)
    nq = 1 if size == "small" else 2048
    _, lower, upper = table_ranges(v, nq)
    rws = [ls.closed(v, sc.INCLUDED, lo, sc.INCLUDED, up, False, TS_MAX) for lo, up in zip(lower, upper)]
    exp, out_rows, raw_runs = ls.arrays(rws)
    sizes = lambda rows: (sum(len(e) for e in rows), sum(len(k) for e in rows for k, _, _ in e),
                          sum(len(x) for e in rows for _, _, x in e))
    with scan_units():
        r, seg, raw, out, st = ss.lsm_scan_raw(view, lower, upper, [sc.INCLUDED] * nq, [sc.INCLUDED] * nq, [TS_MAX] * nq,
                                               0, sub_cap=nq, raw_caps=sizes(raw_runs), out_caps=sizes(out_rows))
    assert st == [*sizes(out_rows), 0, *sizes(raw_runs), len(raw_runs)]
    for f in ls.FIELDS:
        assert r[f].astype(np.uint64).tolist() == exp[f].tolist(), f
    check_stream(out, out_rows, seg)
    assert dev_entries(raw) == [e for run in raw_runs for e in run]


def test_lsm_scan():
    run_sequence(lsm_scan_step)


# ---------------------------------------------------------------- the shared arenas
# sws and cws are arenas whose layout the previous call chose: calls of different families in turn
# on one context, each growing or reusing what the one before left.
def test_sws_arena_across_families():
    with fresh_context():
        files_step("small")
        lsm_scan_step("large")
        open_step("small")
        scan_step("large")
        lsm_get_step("small")


def test_cws_arena_across_families():
    with fresh_context():
        merge_step("small")
        compact_step("large")
        rotation_step("small")
        merge_step("large")
