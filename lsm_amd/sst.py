"""SST container (SURVEY.md §8 f, rows 3 and 4): whole SST files and the memtable flush source.

  MemTable          reference src/mem_table.rs:55-158 (host; the flush source of the encoder)
  mem_runs          memtables (or KV streams) as the memtable runs of an LsmView: one stream, run_start
  sst_files         SsTableBuilder::build (src/table/builder.rs:68-98) for every SST of an encode
                    or compaction, on the device: framed data section, BlockMeta section,
                    meta_offset, bloom filter over farmhash::fingerprint32, bloom_offset
  flush_memtable    force_flush_next_imm_memtable's SST (src/lsm_storage.rs:692-744): memtable ->
                    KV batch -> device encode -> one SST file
  SsTable           SsTable::open / read_block / find_block_idx (src/table.rs:162-257) over a file
                    held in memory; blocks are decoded on the device from the framed data section
                    with the read_block CRC check (lsmblk_decode_batch_ex)
  SstSet            SST files resident in device memory, opened once on the device
                    (lsmblk_sst_open_batch), answering batches of (sst, key, read_ts) point lookups
                    with the entry and its value (lsmblk_sst_get_batch), and batches of
                    (sst, lower, upper) range scans with every version in range
                    (lsmblk_sst_scan_batch), filtered to a reader's view by batch.read_filter; over an
                    LsmView (memtable runs, L0 tables and levels of the set) batches of keys with one answer per
                    key, get_with_ts (lsmblk_lsm_get_batch), and batches of
                    ranges with each range's merged reader's view, scan_with_ts
                    (lsmblk_lsm_scan_batch)

Device work goes through liblsmblk.so; the footer / section parsing here is host logic that mirrors
the reference's own (the CRC-32 of those small sections is zlib's, which is crc32fast's).
"""
import ctypes
import functools
import zlib

import numpy as np
import torch

from . import batch
from ._lib import (LSMBLK_BOUND_EXCLUDED, LSMBLK_BOUND_INCLUDED, LSMBLK_BOUND_UNBOUNDED, LSMBLK_E_CAPACITY,
                   LSMBLK_ERR_CAPACITY, LSMBLK_ERR_OVERFLOW, LSMBLK_GET_FOUND, LSMBLK_GET_MVCC, LSMBLK_GET_NO_FILTER,
                   LSMBLK_LSM_GET_NEWEST, LSMBLK_LSM_SCAN_NEWEST, LSMBLK_LSM_SCAN_STATS_WORDS, LSMBLK_SCAN_MVCC,
                   LSMBLK_SCAN_NO_FILTER, GetResultC, LsmBlkError, LsmGetResultC, LsmScanResultC, LsmViewC, ScanResultC,
                   SstDescC, SstIndexC, check, lib)


class MemTable:
    """MemTable (src/mem_table.rs:55-158): key order ignores the ts, so a put of a present key
    replaces the entry; flush() yields the entries in key order."""

    def __init__(self):
        self.h = lib().lsmblk_memtable_new()
        if not self.h:
            raise MemoryError("lsmblk_memtable_new")

    def __del__(self):
        if getattr(self, "h", None):
            lib().lsmblk_memtable_free(self.h)
            self.h = None

    def put(self, key: bytes, ts: int, value: bytes):
        check(lib().lsmblk_memtable_put(self.h, key, len(key), ts, value, len(value)), "memtable put")

    def get(self, key: bytes):
        """(value, ts) or None; the value is copied under the memtable's lock."""
        n, t = ctypes.c_size_t(), ctypes.c_uint64()
        buf = ctypes.create_string_buffer(256)
        for _ in range(8):  # a concurrent put may grow the value between the size probe and the copy
            found = lib().lsmblk_memtable_get_copy(self.h, key, len(key), buf, len(buf), ctypes.byref(n),
                                                   ctypes.byref(t))
            if found != LSMBLK_E_CAPACITY:
                break
            buf = ctypes.create_string_buffer(max(n.value, 1))
        if found < 0:
            raise LsmBlkError(found, "memtable get")
        return (buf.raw[:n.value], t.value) if found else None

    def __len__(self):
        return lib().lsmblk_memtable_len(self.h)

    def approximate_size(self):
        return lib().lsmblk_memtable_approximate_size(self.h)

    def flush_arrays(self):
        """MemTable::flush (:131-136) -> (keys u8, key_off u32, vals u8, val_off u32, ts u64)."""
        n, K, V = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        lib().lsmblk_memtable_flush(self.h, None, None, None, None, None, 0, 0, 0, ctypes.byref(n), ctypes.byref(K),
                                    ctypes.byref(V))
        keys = np.zeros(max(K.value, 1), np.uint8)
        vals = np.zeros(max(V.value, 1), np.uint8)
        ko = np.zeros(n.value + 1, np.uint32)
        vo = np.zeros(n.value + 1, np.uint32)
        ts = np.zeros(max(n.value, 1), np.uint64)
        check(lib().lsmblk_memtable_flush(self.h, keys.ctypes.data, ko.ctypes.data, vals.ctypes.data, vo.ctypes.data,
                                          ts.ctypes.data, n.value, K.value, V.value, ctypes.byref(n), ctypes.byref(K),
                                          ctypes.byref(V)), "memtable flush")
        return keys[:K.value], ko, vals[:V.value], vo, ts[:n.value]


def fingerprint32(key: bytes) -> int:
    """farmhash::fingerprint32 (src/table/builder.rs:53), the library's restatement."""
    return lib().lsmblk_fingerprint32(key, len(key))


def sst_files_into(blocks, blk_off, nblk, sst_blk, sst_ent, nsst, kv: batch.KVStream, files, files_cap, file_off,
                   stats, stream=None):
    """Whole SST files into a caller's buffer (files may be None with files_cap 0: the size
    alone).  stats[1] = the bytes required; where that exceeds files_cap the stats carry
    CAPACITY and nothing is written.  No host sync of the result: read stats after one."""
    dev = batch._dev_index(blk_off)
    batch._need(blk_off, torch.int64, "blk_off", dev, nblk + 1)
    batch._need(sst_blk, torch.int32, "sst_blk", dev, nsst + 1)
    batch._need(sst_ent, torch.int32, "sst_ent", dev, nsst + 1)
    batch._need(file_off, torch.int64, "file_off", dev, nsst + 1)
    batch._need(stats, torch.int64, "stats", dev, batch.STATS_WORDS)
    if files is not None:
        batch._need(files, torch.uint8, "files", dev, files_cap)
    elif files_cap:
        raise ValueError("files: missing tensor")
    kv.check(dev, "kv")
    c = kv._c()
    batch._native("lsmblk_sst_files_batch", dev, stream, batch._ptr(blocks), blk_off.data_ptr(), nblk,
                  sst_blk.data_ptr(), sst_ent.data_ptr(), nsst, ctypes.byref(c),
                  files.data_ptr() if files is not None else None, files_cap, file_off.data_ptr(),
                  stats.data_ptr(), batch._stream_ptr(stream, dev))


def sst_files(blocks, blk_off, sst_blk, sst_ent, kv: batch.KVStream, stream=None):
    """Whole SST files for every SST (sst_blk / sst_ent: u32 tables of nsst+1) -> (files u8 tensor,
    file_off int64 tensor[nsst+1]); file s = files[file_off[s]:file_off[s+1]]."""
    dev = torch.device("cuda", batch._dev_index(blk_off))
    sst_blk, sst_ent = batch._u32_table(sst_blk, dev), batch._u32_table(sst_ent, dev)
    nsst, nblk = sst_blk.numel() - 1, blk_off.numel() - 1
    file_off = torch.zeros(nsst + 1, dtype=torch.int64, device=dev)
    stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device=dev)
    kb, _ = kv.byte_sizes()
    cap = int(blocks.numel()) + 8 * nblk + 2 * kb + 64 * nsst + 2 * kv.n + 1024
    for _ in range(2):
        files = batch._aligned_empty(cap, dev)
        sst_files_into(blocks, blk_off, nblk, sst_blk, sst_ent, nsst, kv, files, cap, file_off, stats, stream)
        torch.cuda.synchronize(dev)
        st = batch._status(stats)
        if st == -3:
            cap = int(stats[1].item())
            continue
        if st:
            raise LsmBlkError(st, "sst_files")
        return files[:int(stats[1].item())], file_off
    raise LsmBlkError(-3, "sst_files")


def flush_memtable(mt: MemTable, block_size: int = 4096, device="cuda", stream=None) -> bytes:
    """force_flush_next_imm_memtable's SST (src/lsm_storage.rs:692-744): MemTable::flush into one
    SsTableBuilder (one segment), encoded and framed on the device -> the SST file bytes."""
    keys, ko, vals, vo, ts = mt.flush_arrays()
    if len(ts) == 0:
        raise ValueError("flushing an empty memtable builds an empty SST (the reference panics)")
    d = batch.KVStream.from_numpy(keys, ko, vals, vo, ts, device=device)
    r = batch.encode_sst(d, np.array([0, d.n], np.uint32), block_size, stream)
    files, off = sst_files(r["blocks"], r["blk_off"], r["seg_blk"], np.array([0, d.n], np.uint32), d, stream)
    return files.cpu().numpy().tobytes()


class BlockMeta:
    __slots__ = ("offset", "first_key", "last_key")

    def __init__(self, offset, first_key, last_key):
        self.offset, self.first_key, self.last_key = offset, first_key, last_key


def _decode_block_meta(buf: bytes):
    """BlockMeta::decode_block_meta (src/table.rs:65-93)."""
    num = int.from_bytes(buf[0:4], "big")
    if int.from_bytes(buf[-4:], "big") != zlib.crc32(buf[4:-4]):
        raise ValueError("meta checksum mismatched")
    pos, metas = 4, []
    for _ in range(num):
        off = int.from_bytes(buf[pos:pos + 4], "big")
        fl = int.from_bytes(buf[pos + 4:pos + 6], "big")
        fk = bytes(buf[pos + 6:pos + 6 + fl])
        pos += 6 + fl + 8
        ll = int.from_bytes(buf[pos:pos + 2], "big")
        lk = bytes(buf[pos + 2:pos + 2 + ll])
        pos += 2 + ll + 8
        metas.append(BlockMeta(off, fk, lk))
    return metas, int.from_bytes(buf[pos:pos + 8], "big")


class SsTable:
    """SsTable (src/table.rs:136-283) over a whole file in memory (the reference preads it)."""

    def __init__(self, buf: bytes, device="cuda"):
        n = len(buf)
        bloom_offset = int.from_bytes(buf[n - 4:], "big")  # open, :164-168
        raw = buf[bloom_offset:n - 4]
        if int.from_bytes(raw[-4:], "big") != zlib.crc32(raw[:-4]):
            raise ValueError("checksum mismatched for bloom filters")  # bloom.rs:49-54
        self.bloom_filter, self.bloom_k = bytes(raw[:-5]), raw[-5]
        self.block_meta_offset = int.from_bytes(buf[bloom_offset - 4:bloom_offset], "big")  # :170-172
        self.block_meta, self.max_ts = _decode_block_meta(buf[self.block_meta_offset:bloom_offset - 4])
        self.first_key = self.block_meta[0].first_key
        self.last_key = self.block_meta[-1].last_key
        self.buf, self.device = buf, device

    def num_of_blocks(self):
        return len(self.block_meta)

    def find_block_idx(self, key: bytes) -> int:  # :253-257 (partition_point, ts-agnostic)
        lo, hi = 0, len(self.block_meta)
        while lo < hi:
            mid = (lo + hi) // 2
            if self.block_meta[mid].first_key <= key:
                lo = mid + 1
            else:
                hi = mid
        return max(lo - 1, 0)

    def may_contain(self, key: bytes) -> bool:  # bloom.may_contain(fingerprint32(key)), lsm_storage.rs:389-391
        f = self.bloom_filter
        return bool(lib().lsmblk_bloom_may_contain(f, len(f), self.bloom_k, fingerprint32(key)))

    def block_offsets(self):
        """Framed block ranges: BlockMeta offsets, then the meta section (read_block, :215-220)."""
        return np.array([m.offset for m in self.block_meta] + [self.block_meta_offset], np.uint64)

    def decode_blocks(self, lo=0, hi=None, verify=True):
        """read_block for blocks [lo, hi) at once (:213-233): the framed ranges decoded on the
        device with the CRC check -> KVStream."""
        off = self.block_offsets()
        hi = len(self.block_meta) if hi is None else hi
        a, b = int(off[lo]), int(off[hi])
        data = torch.frombuffer(bytearray(self.buf[a:b]), dtype=torch.uint8).to(self.device)
        rel = torch.from_numpy((off[lo:hi + 1] - off[lo]).view(np.int64)).to(self.device)
        return batch.decode_blocks(data, rel, tail=4, verify=verify)


ERR_CAPACITY = LSMBLK_ERR_CAPACITY
GET_FIELDS = ("status", "blk", "ent", "hit_blk", "hit_ent", "vlen", "ts", "val_pos")
LSM_GET_FIELDS = ("status", "src", "sst", "hit_blk", "hit_ent", "vlen", "ts", "val_pos", "seeks", "bloom_out")
SCAN_FIELDS = ("status", "blk0", "ent0", "blk1", "ent1", "blocks", "n")
LSM_SCAN_FIELDS = ("status", "sources", "raw", "merged", "n")
BOUND_KINDS = {"unbounded": LSMBLK_BOUND_UNBOUNDED, "included": LSMBLK_BOUND_INCLUDED, "excluded": LSMBLK_BOUND_EXCLUDED}


def _bound_kind(k):
    return BOUND_KINDS[k] if isinstance(k, str) else int(k)


MAX_MEM_RUNS = 64  # lsmblk_lsm_view.nmem


def mem_runs(sources, device="cuda"):
    """The memtable runs of a view: `sources` in priority order -- the mutable memtable, then the
    immutable ones, newest first -- each a MemTable (through flush_arrays) or a batch.KVStream on the
    device -> (the runs back to back as one KVStream, run_start: an int32 (u32) tensor of
    len(sources) + 1).  Run r is entries [run_start[r], run_start[r + 1])."""
    dev = torch.device(device)
    # per run (keys, key_off, vals, val_off, ts), the arenas trimmed to the run's bytes
    parts = [s.flush_arrays() if isinstance(s, MemTable) else s.to_numpy() for s in sources]
    cat = lambda i, dt: np.concatenate([np.zeros(0, dt)] + [np.asarray(p[i], dt) for p in parts])

    def offsets(i, arena):  # the runs' offsets, each rebased onto its arena's place in the concatenation
        base, out = 0, [np.zeros(1, np.uint64)]
        for p in parts:
            out.append(np.asarray(p[i], np.uint64)[1:] + np.uint64(base))
            base += len(p[arena])
        if base > 0xFFFFFFFF:
            raise ValueError("mem_runs: the runs' bytes do not fit u32 offsets")
        return np.concatenate(out).astype(np.uint32)

    start = np.concatenate([[0], np.cumsum([len(p[4]) for p in parts])]).astype(np.uint32)
    kv = batch.KVStream.from_numpy(cat(0, np.uint8), offsets(1, 0), cat(2, np.uint8), offsets(3, 2), cat(4, np.uint64), device=dev)
    return kv, batch._u32_table(start, dev)


class LsmView:
    """An LSM view of an SstSet on the device (lsmblk_lsm_view): `l0` the L0 tables' ids in priority
    order, `levels` per level its ids in key order, `mem` the memtable runs -- what mem_runs returns,
    or its `sources` -- which the view keeps alive.  The view is checked by every lookup call."""

    def __init__(self, l0, levels, device, mem=None):
        if mem is not None and not (isinstance(mem, tuple) and len(mem) == 2 and isinstance(mem[0], batch.KVStream)):
            mem = mem_runs(mem, device)
        self.mem, self.mem_start_t = mem if mem is not None else (None, None)
        self.nmem = self.mem_start_t.numel() - 1 if mem is not None else 0
        if self.nmem > MAX_MEM_RUNS:
            raise LsmBlkError(-1, "a view takes at most %d memtable runs" % MAX_MEM_RUNS)
        self._mem_c = None
        self.l0 = [int(x) for x in l0]
        self.levels = [[int(x) for x in lv] for lv in levels]
        start = np.concatenate([[0], np.cumsum([len(lv) for lv in self.levels])]).astype(np.uint32)
        flat = [x for lv in self.levels for x in lv]
        # (never empty tensors: their data pointer is null)
        self.l0_t = batch._u32_table(np.array(self.l0 or [0], np.uint32), device)
        self.level_sst_t = batch._u32_table(np.array(flat or [0], np.uint32), device)
        self.level_start_t = batch._u32_table(start, device)

    def _c(self):
        cv = LsmViewC(self.l0_t.data_ptr(), len(self.l0), len(self.levels), self.level_sst_t.data_ptr(),
                      self.level_start_t.data_ptr())
        if self.nmem:
            self._mem_c = self.mem._c()  # (the host struct the view points at lives as long as the view)
            cv.mem, cv.mem_start, cv.nmem = ctypes.pointer(self._mem_c), self.mem_start_t.data_ptr(), self.nmem
        return cv


class SstSet:
    """SST files resident in device memory, opened once on the device (lsmblk_sst_open_batch):
    file s = files[file_off[s]:file_off[s+1]], as sst_files returns them.  `files` is bytes, a numpy
    u8 array or a u8 tensor; `file_off` an int64 tensor or any sequence.  A call-wide error
    (lsmblk_sst_open_batch's stats[3]) raises LsmBlkError; an SST whose open failed keeps its flags
    in err[s] and 0 blocks (lookups against it report ABSENT) while the others answer.  No file at
    all (files empty, file_off [0]) is a valid set: a database that has never flushed, read through
    a view of memtable runs only."""

    def __init__(self, files, file_off, device="cuda", stream=None):
        dev = torch.device(device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device, self.stream = dev, stream
        if not isinstance(files, torch.Tensor):
            files = torch.from_numpy(np.frombuffer(bytes(files), np.uint8).copy() if isinstance(files, (bytes, bytearray))
                                     else np.ascontiguousarray(files, np.uint8))
        if files.device != dev or files.data_ptr() % 16 or not files.is_contiguous():
            t = batch._aligned_empty(files.numel(), dev)
            t[:files.numel()].copy_(files)
            files = t
        if not isinstance(file_off, torch.Tensor):
            file_off = torch.from_numpy(np.ascontiguousarray(file_off, np.uint64).view(np.int64))
        self.files, self.file_off = files, file_off.to(dev).contiguous()
        batch._need(self.file_off, torch.int64, "file_off", dev.index, 1)
        self.nsst = self.file_off.numel() - 1
        self.desc_t = torch.zeros(max(self.nsst, 1) * ctypes.sizeof(SstDescC), dtype=torch.uint8, device=dev)
        self.index_t = None
        cap = 0
        for _ in range(2):  # the first call sizes the block index
            st = self._open(cap)
            if not (st[3] & LSMBLK_ERR_CAPACITY):
                break
            cap = st[1]
            self.index_t = batch._aligned_empty(cap * ctypes.sizeof(SstIndexC), dev)
        self.open_stats = st
        if st[3]:
            raise LsmBlkError(lib().lsmblk_stats_status(st[3]), "sst open")
        self.desc = self.desc_t.cpu().numpy().view(np.dtype(SstDescC))[:self.nsst]
        self.index = (self.index_t[:cap * ctypes.sizeof(SstIndexC)].cpu().numpy().view(np.dtype(SstIndexC))
                      if cap else np.zeros(0, np.dtype(SstIndexC)))
        self.err = self.desc["err"].copy()
        self._host = None

    def _open(self, index_cap):
        stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device=self.device)
        batch._native("lsmblk_sst_open_batch", self.device.index, self.stream, batch._ptr(self.files),
                      self.file_off.data_ptr(), self.nsst, self.desc_t.data_ptr(), batch._ptr(self.index_t),
                      index_cap, stats.data_ptr(), batch._stream_ptr(self.stream, self.device.index))
        torch.cuda.synchronize(self.device)
        return batch._stats_words(stats)

    # ---- what SsTable::open leaves (read back from the descriptors and the index)
    def _file_bytes(self):
        if self._host is None:
            self._host = self.files.cpu().numpy()
        return self._host

    def _slice(self, pos, n):
        return self._file_bytes()[int(pos):int(pos) + int(n)].tobytes()

    def num_of_blocks(self, s):
        return int(self.desc["nblk"][s])

    def first_key(self, s):
        return self._slice(self.desc["first_key_pos"][s], self.desc["first_key_len"][s])

    def last_key(self, s):
        return self._slice(self.desc["last_key_pos"][s], self.desc["last_key_len"][s])

    def max_ts(self, s):
        return int(self.desc["max_ts"][s])

    def bloom_k(self, s):
        return int(self.desc["bloom_k"][s])

    def bloom_filter(self, s):
        return self._slice(self.desc["bloom_pos"][s], self.desc["bloom_len"][s])

    def _records(self, s):
        b0 = int(self.desc["blk0"][s])
        return self.index[b0:b0 + int(self.desc["nblk"][s])]

    def block_offsets(self, s):
        """Framed block ranges of SST s: BlockMeta offsets, then the meta section (as SsTable.block_offsets)."""
        r = self._records(s)
        return np.array(list(r["off"]) + [int(self.desc["meta_offset"][s])] if len(r) else [], np.uint64)

    def block_meta(self, s):
        """[(offset, end, first_key)] per block of SST s."""
        fo = int(self.file_off[s].item())
        return [(int(r["off"]), int(r["end"]), self._slice(fo + int(r["key_pos"]), r["key_len"])) for r in self._records(s)]

    # ---- lookups
    def _set_args(self):
        """The set's leading arguments of every lookup call."""
        return (batch._ptr(self.files), self.file_off.data_ptr(), self.nsst, self.desc_t.data_ptr(),
                batch._ptr(self.index_t))

    def _need_get(self, qkey_off, q_ts, nq, res, res_c, stats, vals, val_cap, val_off):
        """The checks get_into and lsm_get_into share -> the call's (vals, val_cap, val_off) arguments."""
        dev = self.device.index
        batch._need(qkey_off, torch.int32, "qkey_off", dev, nq + 1)
        batch._need(q_ts, torch.int64, "q_ts", dev, nq)
        batch._need(res, torch.uint8, "res", dev, nq * ctypes.sizeof(res_c))
        batch._need(stats, torch.int64, "stats", dev, batch.STATS_WORDS)
        if vals is None:
            return None, 0, None
        batch._need(vals, torch.uint8, "vals", dev, val_cap)
        batch._need(val_off, torch.int32, "val_off", dev, nq + 1)
        return vals.data_ptr(), val_cap, val_off.data_ptr()

    def _get_call(self, res_c, into, nq, val_cap, vals):
        """One point-read call, get_raw's and lsm_get_raw's: `into` is get_into / lsm_get_into bound up
        to `flags`; allocates the results, calls, synchronizes and reads back."""
        dev = self.device
        res = torch.zeros(max(nq, 1) * ctypes.sizeof(res_c), dtype=torch.uint8, device=dev)
        stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device=dev)
        vo = None
        if val_cap is not None:
            if vals is None:
                vals = batch._aligned_empty(val_cap, dev)
            vo = torch.zeros(nq + 1, dtype=torch.int32, device=dev)
        into(res, stats, vals if val_cap is not None else None, val_cap or 0, vo)
        torch.cuda.synchronize(dev)
        r = res.cpu().numpy().view(np.dtype(res_c))[:nq]
        st = batch._stats_words(stats)
        return r, vals, (vo.cpu().numpy().view(np.uint32) if vo is not None else None), st

    def _get(self, raw, nq, fields, what, values):
        """get's and lsm_get's loop: raw(val_cap) is one *_get_raw call; one retry on CAPACITY with the
        bytes it reported, then the dict of the fields and, with `values`, the value bytes."""
        cap = 64 * nq + 1024 if values else None
        for _ in range(2):
            r, vals, vo, st = raw(cap)
            if values and st[3] == LSMBLK_ERR_CAPACITY:
                cap = st[2]
                continue
            break
        if st[3]:
            raise LsmBlkError(lib().lsmblk_stats_status(st[3]), what)
        out = {f: r[f].copy() for f in fields}
        if values:
            hv = vals[:int(vo[-1])].cpu().numpy() if len(vo) else np.zeros(0, np.uint8)
            out["val_off"] = vo
            out["values"] = [hv[vo[i]:vo[i + 1]].tobytes() if r["status"][i] == LSMBLK_GET_FOUND else None
                             for i in range(nq)]
        return out

    def get_into(self, q_sst, qkeys, qkey_off, q_ts, nq, flags, res, stats, vals=None, val_cap=0, val_off=None):
        """Asynchronous lsmblk_sst_get_batch over device tensors (no host sync): q_sst / qkey_off int32
        (u32), q_ts int64 (u64), res uint8[40 nq], stats int64[4]; vals / val_off None: no gather."""
        dev = self.device.index
        batch._need(q_sst, torch.int32, "q_sst", dev, nq)
        tail = self._need_get(qkey_off, q_ts, nq, res, GetResultC, stats, vals, val_cap, val_off)
        batch._native("lsmblk_sst_get_batch", dev, self.stream, *self._set_args(), q_sst.data_ptr(), qkeys.data_ptr(),
                      qkey_off.data_ptr(), q_ts.data_ptr(), nq, flags, res.data_ptr(), *tail, stats.data_ptr(),
                      batch._stream_ptr(self.stream, dev))

    def upload_queries(self, q_sst, keys, read_ts):
        """Host queries -> the device tensors of get_into: (q_sst, qkeys, qkey_off, q_ts)."""
        dev, nq = self.device, len(keys)
        kb = b"".join(bytes(k) for k in keys)
        ko = np.zeros(nq + 1, np.uint32)
        if nq:
            ko[1:] = np.cumsum([len(k) for k in keys])
        qk = batch._aligned_empty(len(kb) + 16, dev)
        if kb:
            qk[:len(kb)].copy_(torch.frombuffer(bytearray(kb), dtype=torch.uint8))
        qs = batch._u32_table(np.ascontiguousarray(q_sst, np.uint32).reshape(-1) if nq else np.zeros(1, np.uint32), dev)
        qt = self._read_ts(read_ts, nq)
        return qs, qk, batch._u32_table(ko, dev), qt

    def _read_ts(self, read_ts, nq):
        """One read_ts for all or one per query -> the int64 (u64) device tensor of nq (never empty)."""
        ts = np.broadcast_to(np.asarray(read_ts, np.uint64), (nq,)).copy() if nq else np.zeros(1, np.uint64)
        return torch.from_numpy(ts.view(np.int64)).to(self.device)

    def get_raw(self, q_sst, keys, read_ts, flags=0, val_cap=None, vals=None):
        """One lsmblk_sst_get_batch call -> (results as a numpy record array, vals tensor or None,
        val_off numpy or None, stats list); nothing raises on the stats.  val_cap None: no gather."""
        nq = len(keys)
        qs, qk, qo, qt = self.upload_queries(q_sst, keys, read_ts)
        return self._get_call(GetResultC, functools.partial(self.get_into, qs, qk, qo, qt, nq, flags), nq, val_cap, vals)

    def get(self, q_sst, keys, read_ts, *, no_filter=False, mvcc=False, values=True):
        """Batched point lookups: query i = (q_sst[i], keys[i], read_ts[i] or the scalar read_ts) ->
        dict of numpy arrays (status, blk, ent, hit_blk, hit_ent, vlen, ts, val_pos; LSMBLK_GET_*
        statuses) and, with `values`, "values": a list of the FOUND lookups' value bytes (None for
        the others) and "val_off"."""
        flags = (LSMBLK_GET_NO_FILTER if no_filter else 0) | (LSMBLK_GET_MVCC if mvcc else 0)
        return self._get(lambda cap: self.get_raw(q_sst, keys, read_ts, flags, cap), len(keys), GET_FIELDS, "sst get",
                         values)

    # ---- point reads over an LSM view
    def view(self, l0, levels, mem=None):
        """An LsmView of this set: l0 = SST ids in priority order, levels = per level its ids in key
        order, mem = the memtable runs (mem_runs' result or its sources; None: a view of tables only)."""
        return LsmView(l0, levels, self.device, mem)

    def lsm_get_into(self, view, qkeys, qkey_off, q_ts, nq, flags, res, stats, vals=None, val_cap=0, val_off=None):
        """Asynchronous lsmblk_lsm_get_batch over device tensors (no host sync): qkey_off int32 (u32),
        q_ts int64 (u64), res uint8[48 nq], stats int64[4]; vals / val_off None: no gather."""
        dev = self.device.index
        tail = self._need_get(qkey_off, q_ts, nq, res, LsmGetResultC, stats, vals, val_cap, val_off)
        cv = view._c()
        batch._native("lsmblk_lsm_get_batch", dev, self.stream, *self._set_args(), ctypes.byref(cv), qkeys.data_ptr(),
                      qkey_off.data_ptr(), q_ts.data_ptr(), nq, flags, res.data_ptr(), *tail, stats.data_ptr(),
                      batch._stream_ptr(self.stream, dev))

    def lsm_get_raw(self, view, keys, read_ts, flags=0, val_cap=None, vals=None):
        """One lsmblk_lsm_get_batch call -> (results as a numpy record array, vals tensor or None,
        val_off numpy or None, stats list); nothing raises on the stats.  val_cap None: no gather."""
        nq = len(keys)
        _, qk, qo, qt = self.upload_queries([0] * nq, keys, read_ts)
        return self._get_call(LsmGetResultC, functools.partial(self.lsm_get_into, view, qk, qo, qt, nq, flags), nq, val_cap,
                              vals)

    def lsm_get(self, view, keys, read_ts, *, mvcc=False, newest=False, values=True):
        """get_with_ts (below the memtables for a view without runs) for a batch of keys: key i at read_ts[i] (or the scalar
        read_ts) over `view` -> dict of numpy arrays (status, src, sst, hit_blk, hit_ent, vlen, ts,
        val_pos, seeks, bloom_out) and, with `values`, "values" (the FOUND keys' value bytes, None for
        the others) and "val_off".  mvcc: the corrected landing per table; newest: the version with
        the largest ts <= read_ts over every source (LSMBLK_LSM_GET_NEWEST)."""
        flags = (LSMBLK_GET_MVCC if mvcc else 0) | (LSMBLK_LSM_GET_NEWEST if newest else 0)
        return self._get(lambda cap: self.lsm_get_raw(view, keys, read_ts, flags, cap), len(keys), LSM_GET_FIELDS, "lsm get",
                         values)

    # ---- range scans
    def _need_ranges(self, lkey_off, ukey_off, q_bound, q_ts, nq, res, res_c, seg_start, stats, stats_words):
        """The checks scan_into and lsm_scan_into share (q_ts None: the call takes none, or none is given)."""
        dev = self.device.index
        batch._need(lkey_off, torch.int32, "lkey_off", dev, nq + 1)
        batch._need(ukey_off, torch.int32, "ukey_off", dev, nq + 1)
        batch._need(q_bound, torch.int32, "q_bound", dev, nq)
        if q_ts is not None:
            batch._need(q_ts, torch.int64, "q_ts", dev, nq)
        batch._need(res, torch.uint8, "res", dev, nq * ctypes.sizeof(res_c))
        batch._need(seg_start, torch.int32, "seg_start", dev, nq + 1)
        batch._need(stats, torch.int64, "stats", dev, stats_words)

    def _stream_arg(self, s, caps, name):
        """An output stream or None -> the call's argument: its C struct with `caps` (default s.caps())."""
        if s is None:
            return None
        s.check(self.device.index, name, 0)
        return ctypes.byref(s._c(*(caps if caps is not None else s.caps())))

    @staticmethod
    def _rows(kv, seg, nq):
        """Per range q its entries [seg[q], seg[q + 1]) of kv as (key, ts, value)."""
        keys, ko, vals, vo, ts = kv.to_numpy()
        kb, vb = keys.tobytes(), vals.tobytes()
        return [[(kb[ko[i]:ko[i + 1]], int(ts[i]), vb[vo[i]:vo[i + 1]]) for i in range(int(seg[q]), int(seg[q + 1]))]
                for q in range(nq)]

    def scan_into(self, q_sst, lkeys, lkey_off, ukeys, ukey_off, q_bound, nq, flags, res, seg_start, stats,
                  out: batch.KVStream = None, caps=None):
        """Asynchronous lsmblk_sst_scan_batch over device tensors (no host sync): q_sst / lkey_off /
        ukey_off / q_bound / seg_start int32 (u32), res uint8[32 nq], stats int64[4]; out None: res,
        seg_start and the sizes in stats only; caps = (entry_cap, key_cap, val_cap), default out.caps()."""
        dev = self.device.index
        batch._need(q_sst, torch.int32, "q_sst", dev, nq)
        self._need_ranges(lkey_off, ukey_off, q_bound, None, nq, res, ScanResultC, seg_start, stats, batch.STATS_WORDS)
        batch._native("lsmblk_sst_scan_batch", dev, self.stream, *self._set_args(), q_sst.data_ptr(), lkeys.data_ptr(),
                      lkey_off.data_ptr(), ukeys.data_ptr(), ukey_off.data_ptr(), q_bound.data_ptr(), nq, flags,
                      res.data_ptr(), self._stream_arg(out, caps, "out"), seg_start.data_ptr(), stats.data_ptr(),
                      batch._stream_ptr(self.stream, dev))

    def upload_ranges(self, q_sst, lower, upper, lower_kind, upper_kind):
        """Host ranges -> the device tensors of scan_into: (q_sst, lkeys, lkey_off, ukeys, ukey_off,
        q_bound).  A kind is one per range or one for all: "unbounded" / "included" / "excluded" or
        LSMBLK_BOUND_*; an unbounded side's key may be None."""
        nq = len(lower)
        kinds = lambda k: [_bound_kind(x) for x in k] if isinstance(k, (list, tuple, np.ndarray)) else [_bound_kind(k)] * nq
        bnd = np.array([a | (b << 2) for a, b in zip(kinds(lower_kind), kinds(upper_kind))] or [0], np.uint32)
        qs, lk, lo, _ = self.upload_queries(q_sst, [k or b"" for k in lower], 0)
        _, uk, uo, _ = self.upload_queries(q_sst, [k or b"" for k in upper], 0)
        return qs, lk, lo, uk, uo, batch._u32_table(bnd, self.device)

    def scan_raw(self, q_sst, lower, upper, lower_kind, upper_kind, flags=0, caps=None, out=None):
        """One lsmblk_sst_scan_batch call -> (results as a numpy record array, seg_start numpy, the
        KVStream or None, stats list); nothing raises on the stats.  caps = (entries, key bytes, value
        bytes) of a fresh output stream (or of `out`, a caller's stream); None: sizes only."""
        dev, nq = self.device, len(lower)
        t = self.upload_ranges(q_sst, lower, upper, lower_kind, upper_kind)
        res = torch.zeros(max(nq, 1) * ctypes.sizeof(ScanResultC), dtype=torch.uint8, device=dev)
        seg = torch.zeros(nq + 1, dtype=torch.int32, device=dev)
        stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device=dev)
        if caps is not None and out is None:
            out = batch.KVStream.empty(*caps, dev)
        self.scan_into(*t, nq, flags, res, seg, stats, out if caps is not None else None, caps)
        torch.cuda.synchronize(dev)
        r = res.cpu().numpy().view(np.dtype(ScanResultC))[:nq]
        st = batch._stats_words(stats)
        if caps is not None and not st[3] & (LSMBLK_ERR_CAPACITY | LSMBLK_ERR_OVERFLOW):
            out.n = st[0]
        return r, seg.cpu().numpy().view(np.uint32), (out if caps is not None else None), st

    def scan(self, q_sst, lower, upper, *, lower_kind, upper_kind, read_ts=None, no_filter=False, mvcc=False):
        """Batched range scans: range i = SST q_sst[i], (lower[i], upper[i]) with the bound kinds ->
        (dict of numpy arrays: status, blk0, ent0, blk1, ent1, blocks, n; LSMBLK_SCAN_* statuses, and
        per range the list of (key, ts, value)).  read_ts None: every version in range (the raw scan);
        else what a reader at read_ts (one for all, or one per range) sees of each range
        (lsmblk_read_filter_batch).  Retries once on CAPACITY with the reported sizes."""
        flags = (LSMBLK_SCAN_NO_FILTER if no_filter else 0) | (LSMBLK_SCAN_MVCC if mvcc else 0)
        nq = len(lower)
        caps = (64 * nq + 1024, 1024 * nq + 4096, 4096 * nq + 4096)
        for _ in range(2):
            r, seg, kv, st = self.scan_raw(q_sst, lower, upper, lower_kind, upper_kind, flags, caps)
            if st[3] == LSMBLK_ERR_CAPACITY:
                caps = (st[0], st[1], st[2])
                continue
            break
        if st[3]:
            raise LsmBlkError(lib().lsmblk_stats_status(st[3]), "sst scan")
        if read_ts is not None and nq:
            kv, seg = batch.read_filter(kv, seg, read_ts, self.stream)
        return {f: r[f].copy() for f in SCAN_FIELDS}, self._rows(kv, seg, nq)

    # ---- range scans over an LSM view
    def lsm_scan_into(self, view, lkeys, lkey_off, ukeys, ukey_off, q_bound, q_ts, nq, flags, sub_cap, res, seg_start,
                      stats, raw: batch.KVStream = None, out: batch.KVStream = None, raw_caps=None, out_caps=None):
        """Asynchronous lsmblk_lsm_scan_batch over device tensors (no host sync): lkey_off / ukey_off /
        q_bound / seg_start int32 (u32), q_ts int64 (u64) or None (the merged stream), res uint8[32 nq],
        stats int64[8]; raw None: the table scans are sized only; out None: sizes only; *_caps =
        (entry_cap, key_cap, val_cap), default the stream's caps()."""
        dev = self.device.index
        self._need_ranges(lkey_off, ukey_off, q_bound, q_ts, nq, res, LsmScanResultC, seg_start, stats,
                          LSMBLK_LSM_SCAN_STATS_WORDS)
        craw, cout = self._stream_arg(raw, raw_caps, "raw"), self._stream_arg(out, out_caps, "out")
        cv = view._c()
        batch._native("lsmblk_lsm_scan_batch", dev, self.stream, *self._set_args(), ctypes.byref(cv), lkeys.data_ptr(),
                      lkey_off.data_ptr(), ukeys.data_ptr(), ukey_off.data_ptr(), q_bound.data_ptr(),
                      q_ts.data_ptr() if q_ts is not None else None, nq, flags, sub_cap, res.data_ptr(), craw, cout,
                      seg_start.data_ptr(), stats.data_ptr(), batch._stream_ptr(self.stream, dev))

    def lsm_scan_raw(self, view, lower, upper, lower_kind, upper_kind, read_ts=None, flags=0, sub_cap=None,
                     raw_caps=None, out_caps=None, raw=None, out=None):
        """One lsmblk_lsm_scan_batch call -> (results as a numpy record array, seg_start numpy, the raw
        KVStream or None, the out KVStream or None, stats list); nothing raises on the stats.
        *_caps = (entries, key bytes, value bytes) of a fresh stream (or of `raw` / `out`, a caller's
        stream); None: that stream is not passed.  sub_cap None: view_sub_cap(view, nq)."""
        dev, nq = self.device, len(lower)
        _, lk, lo, uk, uo, bnd = self.upload_ranges([0] * nq, lower, upper, lower_kind, upper_kind)
        qt = self._read_ts(read_ts, nq) if read_ts is not None else None
        res = torch.zeros(max(nq, 1) * ctypes.sizeof(LsmScanResultC), dtype=torch.uint8, device=dev)
        seg = torch.zeros(nq + 1, dtype=torch.int32, device=dev)
        stats = torch.zeros(LSMBLK_LSM_SCAN_STATS_WORDS, dtype=torch.int64, device=dev)
        if raw_caps is not None and raw is None:
            raw = batch.KVStream.empty(*raw_caps, dev)
        if out_caps is not None and out is None:
            out = batch.KVStream.empty(*out_caps, dev)
        raw = raw if raw_caps is not None else None
        out = out if out_caps is not None else None
        self.lsm_scan_into(view, lk, lo, uk, uo, bnd, qt, nq, flags, view_sub_cap(view, nq) if sub_cap is None else sub_cap,
                           res, seg, stats, raw, out, raw_caps, out_caps)
        torch.cuda.synchronize(dev)
        r = res.cpu().numpy().view(np.dtype(LsmScanResultC))[:nq]
        st = batch._stats_words(stats)
        if not st[3] & (LSMBLK_ERR_CAPACITY | LSMBLK_ERR_OVERFLOW):
            if raw is not None:
                raw.n = st[4]
            if out is not None:
                out.n = st[0]
        return r, seg.cpu().numpy().view(np.uint32), raw, out, st

    def lsm_scan(self, view, lower, upper, *, lower_kind, upper_kind, read_ts=None, mvcc=False, sub_cap=None,
                 newest=False):
        """scan_with_ts (below the memtables for a view without runs) for a batch of ranges over `view`: range i = (lower[i],
        upper[i]) with the bound kinds, at read_ts[i] (or the scalar read_ts) -> (dict of numpy arrays:
        status, sources, raw, merged, n; and per range the list of (key, ts, value)).  read_ts None:
        the merged stream, every version of every key's owning table.  newest
        (LSMBLK_LSM_SCAN_NEWEST, which implies mvcc): the snapshot scan -- the runs merged by (key
        ascending, ts descending), so per key the row is the newest version at or below read_ts over
        every source, as lsm_get(newest=True) gives for one key; with read_ts None the rows are every
        version of every key from every passing table, in that order.  sub_cap defaults to every table
        of the view for every range, which always fits.  Retries at most once on CAPACITY, relying on
        which stats words the header declares valid: a short sub_cap reports only [7], a short raw
        stream [4..7], a short out stream every word (out never needs more than raw)."""
        nq = len(lower)
        cap = view_sub_cap(view, nq) if sub_cap is None else sub_cap
        rc = oc = (64 * nq + 1024, 1024 * nq + 4096, 4096 * nq + 4096)
        flags = (LSMBLK_SCAN_MVCC if mvcc else 0) | (LSMBLK_LSM_SCAN_NEWEST if newest else 0)
        for _ in range(2):
            r, seg, _, kv, st = self.lsm_scan_raw(view, lower, upper, lower_kind, upper_kind, read_ts, flags, cap, rc, oc)
            if st[3] != LSMBLK_ERR_CAPACITY:
                break
            if st[7] > cap:  # no scan ran: the streams' sizes are still unknown
                cap = st[7]
            elif st[4] > rc[0] or st[5] > rc[1] or st[6] > rc[2]:
                rc = (st[4], st[5], st[6])
                oc = tuple(max(a, b) for a, b in zip(oc, rc))
            else:
                oc = (st[0], st[1], st[2])
        if st[3]:
            raise LsmBlkError(lib().lsmblk_stats_status(st[3]), "lsm scan")
        return {f: r[f].copy() for f in LSM_SCAN_FIELDS}, self._rows(kv, seg, nq)


def open_compacted(r, device="cuda", stream=None):
    """The SSTs of a batch.compact_runs result as files, opened: (SstSet, its one-level LsmView) --
    what a reader sees once the compaction's output has replaced its inputs."""
    files, off = sst_files(r["blocks"], r["blk_off"], r["sst_blk"], r["sst_start"], r["kept"], stream)
    ss = SstSet(files, off, device, stream)
    return ss, ss.view([], [list(range(ss.nsst))])


def view_sub_cap(view, nq):
    """Table scans a batch of nq ranges over the view can expand into at most: every memtable run and
    every table, every range."""
    return nq * (view.nmem + len(view.l0) + sum(len(lv) for lv in view.levels))
