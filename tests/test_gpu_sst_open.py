"""lsmblk_sst_open_batch on the device against the open rule of open_cases.py: every descriptor field,
every index record and stats[0..3], exactly, for files that put each field of the walk on each split
of its LDS window's end at every 16-byte residue of the file start, keys of up to 65535 bytes, a file
on each side of every bounds check, section CRC flips, and batches whose failed SSTs shift the slots
of the SSTs after them.

Every call gets its files between two guard regions at a 16-byte-aligned view of a larger buffer, and
`desc` / `index` inside longer pattern-filled tensors with index_cap exactly the required count: what
lies outside a file must not matter, and what lies outside desc[0 .. nsst) and index[0 .. stats[1])
must keep its pattern.  For a failed SST only err, nblk == 0 and blk0 are compared: its other
descriptor fields and its index slots are unspecified."""
import ctypes

import numpy as np
import pytest
import torch

import get_cases as gc
import open_cases as oc
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch, sst
from lsm_amd._lib import SstDescC, SstIndexC
from oracle import pyref

pytestmark = pytest.mark.gpu

GUARD = 4096          # bytes before the files' view and after the last file
PAT_DESC, PAT_INDEX = 0xC7, 0x5B
DESC_B, INDEX_B = ctypes.sizeof(SstDescC), ctypes.sizeof(SstIndexC)
PAD_REC = 2           # pattern records before and after desc / index


@pytest.fixture(scope="module")
def meta_bytes():
    """The BlockMeta section of a valid SST: the fill that looks most like what the walk reads."""
    buf = gc.case("bs128").ssts[0].buf
    bo = int.from_bytes(buf[-4:], "big")
    mo = int.from_bytes(buf[bo - 4:bo], "big")
    return np.frombuffer(buf[mo:bo - 4], np.uint8)


def tiled(fill, n):
    if isinstance(fill, int):
        return np.full(n, fill, np.uint8)
    return np.resize(fill, n) if n else np.zeros(0, np.uint8)


class Opened:
    """One lsmblk_sst_open_batch call: the files blob (with its leading junk) at offset GUARD of a
    device buffer filled with `fill`; `data_fill` overwrites the data section of every SST the rule
    opens.  Keeps the tensors so that a second call can reuse them."""

    def __init__(self, blob, file_off, fill=0x00, data_fill=None, index_cap=None):
        dev = torch.device("cuda", torch.cuda.current_device())
        self.dev, self.file_off, self.nsst = dev, [int(x) for x in file_off], len(file_off) - 1
        self.rule = oc.open_batch_rule(blob, self.file_off)
        host = tiled(fill, GUARD + max(len(blob), max(self.file_off)) + GUARD)
        host[GUARD:GUARD + len(blob)] = np.frombuffer(blob, np.uint8)
        host[GUARD:GUARD + min(self.file_off)] = tiled(fill, min(self.file_off))  # the bytes before the first file too
        if data_fill is not None and self.rule["desc"] is not None:
            for s, d in enumerate(self.rule["desc"]):
                if not d["err"]:
                    a = GUARD + self.file_off[s]
                    host[a:a + d["meta_offset"]] = tiled(data_fill, d["meta_offset"])
        self.host = host
        self.buf = batch._aligned_empty(len(host), dev)
        self.buf.copy_(torch.from_numpy(host))
        self.files = self.buf[GUARD:]
        assert self.files.data_ptr() % 16 == 0
        self.off_t = torch.tensor(self.file_off, dtype=torch.int64, device=dev)
        self.need = self.rule["reserved"] if self.rule["reserved"] is not None else 0
        self.cap = self.need if index_cap is None else index_cap
        self.desc_t = torch.full(((self.nsst + 2 * PAD_REC) * DESC_B,), PAT_DESC, dtype=torch.uint8, device=dev)
        self.index_t = torch.full(((self.need + 2 * PAD_REC) * INDEX_B,), PAT_INDEX, dtype=torch.uint8, device=dev)
        assert self.index_t.data_ptr() % 16 == 0
        self.call(self.cap)

    def call(self, cap):
        stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device=self.dev)
        batch._native("lsmblk_sst_open_batch", self.dev.index, None, self.files.data_ptr(), self.off_t.data_ptr(), self.nsst,
                      self.desc_t[PAD_REC * DESC_B:].data_ptr(), self.index_t[PAD_REC * INDEX_B:].data_ptr(), cap,
                      stats.data_ptr(), batch._stream_ptr(None, self.dev.index))
        torch.cuda.synchronize(self.dev)
        self.stats = [int(x) & oc.ALL_ONES for x in stats.cpu().tolist()]
        self.desc_raw = self.desc_t.cpu().numpy()
        self.index_raw = self.index_t.cpu().numpy()
        self.desc = self.desc_raw[PAD_REC * DESC_B:(PAD_REC + self.nsst) * DESC_B].view(np.dtype(SstDescC))
        self.index = self.index_raw[PAD_REC * INDEX_B:(PAD_REC + self.need) * INDEX_B].view(np.dtype(SstIndexC))
        return self.stats

    def check_patterns(self, index_written=None):
        """Nothing outside desc[0 .. nsst) and index[0 .. index_written) was touched."""
        n = self.need if index_written is None else index_written
        d, x = self.desc_raw, self.index_raw
        assert (d[:PAD_REC * DESC_B] == PAT_DESC).all() and (d[(PAD_REC + self.nsst) * DESC_B:] == PAT_DESC).all()
        assert (x[:PAD_REC * INDEX_B] == PAT_INDEX).all() and (x[(PAD_REC + n) * INDEX_B:] == PAT_INDEX).all()

    def check(self, what=""):
        """Every field of every opened SST, err / nblk / blk0 of every failed one, the stats, the patterns."""
        r = self.rule
        assert self.stats == r["stats"], (what, self.stats, r["stats"])
        for s, want in enumerate(r["desc"]):
            got = {f: int(self.desc[f][s]) for f in oc.DESC_FIELDS}
            if want["err"]:  # a failed SST: the rest of its descriptor and its index slots are unspecified
                assert (got["err"], got["nblk"], got["blk0"]) == (want["err"], 0, want["blk0"]), (what, s, got, want)
                continue
            assert got == want, (what, s, got, want)
            for b in range(want["nblk"]):
                slot = want["blk0"] + b
                rec = {f: int(self.index[f][slot]) for f in oc.INDEX_FIELDS}
                assert rec == r["index"][slot], (what, s, b, rec, r["index"][slot])
        self.check_patterns()

    def results(self):
        """What the rule specifies, with positions relative to the first file: comparable between
        calls that differ in what lies outside the files."""
        out = [self.stats]
        for s, want in enumerate(self.rule["desc"]):
            got = {f: int(self.desc[f][s]) for f in oc.DESC_FIELDS}
            if want["err"]:
                out.append((got["err"], got["nblk"], got["blk0"]))
                continue
            for f in ("bloom_pos", "first_key_pos", "last_key_pos"):
                got[f] -= self.file_off[0]
            out.append((got, self.index[want["blk0"]:want["blk0"] + want["nblk"]].tobytes()))
        return out


def open_files(bufs, start=0, **kw):
    blob, off = oc.batch_layout(oc.Batch("", list(bufs), start, None))
    return Opened(blob, off, **kw)


# ------------------------------------------------------------------------------ the window
@pytest.mark.parametrize("kind", oc.KINDS)
def test_every_field_on_every_split_of_the_window_end(kind):
    """Per residue one batch: every file is a multiple of 16 long, so each starts at the residue it
    was built for."""
    for residue in range(16):
        files = oc.straddle_files(kind, residue)
        o = open_files([f.buf for f in files], start=residue, fill=0xEE)
        assert o.stats[0] == len(files) and all(x % 16 == residue for x in o.file_off[:-1])
        o.check((kind, residue))


def test_long_empty_and_image_boundary_keys_at_every_residue():
    files = oc.long_key_files()
    for residue in range(16):
        o = open_files([b for _, b in files], start=residue, fill=0x11 * residue)
        assert o.stats[0] == len(files)
        o.check(("long", residue))


# ------------------------------------------------------------------------------ the edges
def check_alone_and_between(label, buf, start):
    alone = open_files([buf], start=start, fill=0xA5)
    alone.check((label, "alone"))
    left, right = oc.healthy(11), oc.healthy(12)
    mid = open_files([left, buf, right], start=start, fill=0xA5)
    mid.check((label, "middle"))
    # both neighbours open with all their records, and the one after starts past the middle's reserved slots
    err, slots = oc.open_rule(buf)[:2]
    assert [int(e) for e in mid.desc["err"]] == [0, err, 0]
    assert [int(b) for b in mid.desc["blk0"]] == [0, 4, 4 + slots] and int(mid.desc["nblk"][2]) == 1
    assert mid.stats == [2 + (err == 0), 5 + slots, err, 0]


def test_both_sides_of_every_bounds_check():
    assert oc.open_rule(oc.healthy(11))[1] == 4 and oc.open_rule(oc.healthy(12))[1] == 1
    for i, e in enumerate(oc.edge_files()):
        if e.edge != "file_length":
            check_alone_and_between((e.edge, e.side, i), e.buf, start=i % 16)


@pytest.mark.parametrize("fill", range(3))
def test_every_file_length_below_the_smallest_valid_file(fill):
    short = [e for e in oc.edge_files() if e.edge == "file_length"]
    check_alone_and_between("smallest", short[0].buf, start=7)
    for e in short[1 + fill::3]:
        check_alone_and_between(("length", len(e.buf), fill), e.buf, start=len(e.buf) % 16)


def test_section_crc_flips():
    for i, (label, buf, want) in enumerate(oc.crc_files()):
        assert oc.open_rule(buf)[0] == want
        check_alone_and_between(label, buf, start=(5 * i) % 16)


# ------------------------------------------------------------------------------ batches
@pytest.mark.parametrize("b", [b for b in oc.batches() if b.file_off is None], ids=lambda b: b.name)
def test_batches_with_failed_ssts_of_both_kinds(b):
    blob, off = oc.batch_layout(b)
    o = Opened(blob, off, fill=0x3C)
    o.check(b.name)
    need = o.need
    if need:
        # one slot short: CAPACITY, the requirement, nothing opened, the index untouched
        before = o.index_raw.copy()
        st = o.call(need - 1)
        assert st[3] == oc.ERR_CAPACITY and st[1] == need and st[0] == 0
        assert st == oc.open_batch_rule(blob, off, need - 1)["stats"][:2] + [st[2], oc.ERR_CAPACITY]
        assert (o.index_raw == before).all()   # the first call's records are still there
        fresh = Opened(blob, off, fill=0x3C, index_cap=need - 1)
        assert fresh.stats[3] == oc.ERR_CAPACITY and fresh.stats[1] == need and fresh.stats[0] == 0
        assert (fresh.index_raw == PAT_INDEX).all()
        fresh.check_patterns(0)
        # the same context, the same tensors, the exact capacity
        fresh.call(need)
        fresh.check(b.name + " after CAPACITY")


def test_decreasing_file_off_fails_the_call():
    (b,) = [b for b in oc.batches() if b.file_off is not None]
    blob, off = oc.batch_layout(b)
    o = Opened(blob, off)
    # only the call-wide flag and that nothing opened are specified
    assert o.stats[3] == oc.ERR_MALFORMED and o.stats[0] == 0
    o.check_patterns(0)


# ------------------------------------------------------------------------------ bytes outside a file
def test_bytes_outside_the_files_and_in_the_data_sections_do_not_matter(meta_bytes):
    bufs = [f.buf for f in oc.straddle_files("header", 5)[:4]] + [oc.healthy(3), oc.walk_failed(0), oc.prep_refused(0), b"",
                                                                oc.healthy(4), dict(oc.long_key_files())["empty-all"]]
    bufs += [b for _, b, _ in oc.crc_files()]
    base = None
    for start in (5, 26):
        for fill in (0x00, 0xFF, meta_bytes):
            o = open_files(bufs, start=start, fill=fill, data_fill=fill)
            o.check(("fill", start))
            if base is None:
                base = o.results()
            assert o.results() == base, (start, "fill")
    # the data section of a file that the rule fails, too: its verdict and its slots stay
    for fill in (0x00, 0xFF, meta_bytes):
        for buf in (oc.walk_failed(0), oc.walk_failed(2)):
            b = bytearray(buf)
            b[:64] = tiled(fill, 64).tobytes()   # data_len 64
            assert oc.open_rule(bytes(b))[:2] == oc.open_rule(buf)[:2]
            open_files([oc.healthy(1), bytes(b), oc.healthy(2)], start=3, fill=fill).check("failed, data filled")


# ------------------------------------------------------------------------------ reads after the open
def entries_of(lengths, seed):
    """One key per length, two versions each (the older a tombstone for every third; one version for a
    key of two windows or more, to keep the file small), values small: at block_size 4096 a long key
    is alone in its block, so it is a first key and a last key of the BlockMeta section."""
    rng = np.random.default_rng(seed)
    keys = sorted({bytes(rng.integers(97, 123, n, dtype=np.uint8)) for n in lengths if n})
    out = []
    for i, k in enumerate(keys):
        out.append((k, 9, b"new-%d" % i))
        if len(k) < 2 * oc.kOpenChunk:
            out.append((k, 4, b"" if i % 3 == 0 else b"old-%d" % i))
    return out


@pytest.mark.parametrize("which", ["straddle", "long"])
def test_point_reads_over_the_index_the_window_produced(which):
    if which == "straddle":
        every = sorted({len(k) for f in oc.straddle_files("key", 9) for m in pyref.sst_open(f.buf)[0] for k in m[1:]})
        short, long = [n for n in every if n < 64], [n for n in every if n >= 64]
        assert short and len(long) >= 6 and min(long) > oc.kOpenChunk - 256
        lens = [x for pair in zip(short[:6], long[::len(long) // 6]) for x in pair]
        groups = [(lens, 4096), (lens[1::2] + lens[:1], 256)]
    else:
        lens = list(oc.LONG_LENS) + [1, 15, 16, 17]
        groups = [(lens[::2], 4096), (lens[1::2], 256)]
    ssts = [gc.make_sst(entries_of(g, 5 + i), bs) for i, (g, bs) in enumerate(groups)]
    assert all(len(s.buf) <= 300 << 10 for s in ssts)
    # BlockMeta sections of more than one window, at a file start that is no multiple of 16
    assert all(int.from_bytes(s.buf[-4:], "big") - s.meta_offset > oc.kOpenChunk for s in ssts)
    start = 11
    files = oc.junk(start) + b"".join(s.buf for s in ssts)
    off = [start, start + len(ssts[0].buf), start + len(ssts[0].buf) + len(ssts[1].buf)]
    ss = sst.SstSet(files, off)
    assert ss.open_stats == oc.open_batch_rule(files, off)["stats"] and ss.err.tolist() == [0, 0]
    q_sst, keys, read_ts = [], [], []
    for i, s in enumerate(ssts):
        present = sorted({k for k, _, _ in s.entries})
        for k in present + [k[:-1] + b"~" for k in present] + [k + b"a" for k in present[:8]] + [b"A", b"~~"]:
            for ts in (3, 4, 9, 100):
                q_sst.append(i)
                keys.append(k)
                read_ts.append(ts)
    got = ss.get(q_sst, keys, read_ts, mvcc=True)
    rows = [gc.lookup(ssts[s], k, ts, False, True) for s, k, ts in zip(q_sst, keys, read_ts)]
    for f in gc.FIELDS:
        if f == "val_pos":
            want = [0 if r[f] is None else off[s] + r[f] for r, s in zip(rows, q_sst)]
        else:
            want = [r[f] for r in rows]
        bad = np.nonzero(got[f].astype(np.uint64) != np.array(want, np.uint64))[0]
        assert not len(bad), (f, bad[:5], [len(keys[i]) for i in bad[:5]])
    assert got["values"] == [r["value"] for r in rows]
    assert sum(r["status"] == gc.FOUND for r in rows) > len(lens) and sum(r["status"] == gc.TOMBSTONE for r in rows) > 2
