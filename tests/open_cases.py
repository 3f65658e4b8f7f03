"""SST files that reach chosen paths of lsmblk_sst_open_batch -- TEST INFRASTRUCTURE.

The method of path_cases.py / crc_cases.py / sst_cases.py for the open (sst_open_prep_kernel,
sst_open_walk_kernel in lsmblk_get.hip); shared by test_open_cases.py (CPU: the rule agrees with
pyref, the generators reach what they were built for) and test_gpu_sst_open.py (GPU: every descriptor
field, index record and stats word against the rule).

  craft         an SST file assembled byte by byte from explicit parts; the open never reads block
                bytes, so the data section is junk and a BlockMeta section of tens of KB costs a file
                of tens of KB
  open_rule     what lsmblk_sst_open_batch must make of one file, written from include/lsmblk.h
                (lsmblk_sst_desc, lsmblk_sst_index, lsmblk_sst_open_batch) and SsTable::open /
                decode_block_meta; open_batch_rule is the same for a batch, with the slot prefix sums
                and the call-wide flags
  window_trace  the walk's LDS window restated ONLY to classify which field crosses which window end;
                no expected value comes from it
  constants     kOpenChunk, kMetaRecMin read out of the kernel source
"""
import os
import struct
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

import path_cases as pc
from oracle import pyref

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsm_amd", "csrc", "lsmblk_get.hip")
_K = pc.read_constants(_SRC, ("kOpenChunk", "kMetaRecMin"))
kOpenChunk, kMetaRecMin = _K["kOpenChunk"], _K["kMetaRecMin"]

ERR_MALFORMED, ERR_CAPACITY, ERR_CHECKSUM = 1, 2, 128
IMG_BYTES = 16
DESC_FIELDS = ("blk0", "nblk", "meta_offset", "bloom_len", "bloom_pos", "first_key_pos", "last_key_pos",
               "first_key_len", "last_key_len", "max_ts", "bloom_k", "err")
INDEX_FIELDS = ("img_hi", "img_lo", "off", "end", "key_pos", "key_len")
ALL_ONES = 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------ the file writer
def junk(n, salt=7):
    """n bytes that are no SST section (the data section: the open never reads it)."""
    return ((np.arange(n, dtype=np.uint32) * 131 + salt) & 0xFF).astype(np.uint8).tobytes()


def record(off, first_key, last_key, first_ts=0, last_ts=0):
    """One BlockMeta record: u32 offset | u16 | first key | u64 ts | u16 | last key | u64 ts."""
    return (struct.pack(">IH", off & 0xFFFFFFFF, len(first_key)) + first_key + struct.pack(">QH", first_ts, len(last_key)) +
            last_key + struct.pack(">Q", last_ts))


def craft(metas, max_ts=0, bloom=(b"", 1), data_len=64, *, num=None, meta_offset=None, bloom_offset=None,
          meta_crc=None, bloom_crc=None, pad=b"", data=None):
    """data | u32 num | records | u64 max_ts | u32 crc | u32 meta_offset | filter | k | u32 crc |
    u32 bloom_offset.  metas: per record (off, first_key, last_key[, first_ts, last_ts]) or its raw
    bytes; bloom = (filter bytes, k); pad: bytes between the last record and max_ts.  Both CRCs are
    correct unless overridden; num, the offsets and the CRCs take explicit values."""
    body = b"".join(m if isinstance(m, bytes) else record(*m) for m in metas) + pad + struct.pack(">Q", max_ts)
    data = junk(data_len) if data is None else data
    buf = data + struct.pack(">I", (len(metas) if num is None else num) & 0xFFFFFFFF) + body
    buf += struct.pack(">I", zlib.crc32(body) if meta_crc is None else meta_crc)
    buf += struct.pack(">I", len(data) if meta_offset is None else meta_offset)
    sect = bloom[0] + bytes([bloom[1]])
    tail = sect + struct.pack(">I", zlib.crc32(sect) if bloom_crc is None else bloom_crc)
    return buf + tail + struct.pack(">I", len(buf) if bloom_offset is None else bloom_offset)


def craft16(metas, **kw):
    """craft with the filter sized so that the file's length is a multiple of 16: files of a batch
    then all start at the residue of the first."""
    n = len(craft(metas, bloom=(b"", 3), **kw))
    return craft(metas, bloom=(junk((-n) % 16, 99), 3), **kw)


# ------------------------------------------------------------------------------ the rule
def image_ints(key):
    im = key[:IMG_BYTES].ljust(IMG_BYTES, b"\0")
    return int.from_bytes(im[:8], "big"), int.from_bytes(im[8:], "big")


def _u32(buf, p):
    return struct.unpack_from(">I", buf, p)[0]


def open_rule(buf):
    """(err_flags, reserved_slots, desc_fields, index_records) of one file; positions file-relative
    (open_batch_rule makes the descriptor's absolute).  desc_fields / index_records are None where
    the open fails: a failed SST's other fields and its index slots are unspecified.

    A file whose footers or block count are implausible is MALFORMED and reserves nothing; its
    sections cannot be told apart, so no CRC is reported for it.  Otherwise the claimed count is
    reserved, err is CHECKSUM for either section's CRC, OR MALFORMED for the record walk."""
    n = len(buf)
    refused = (ERR_MALFORMED, 0, None, None)
    if n < 4:
        return refused
    bo = _u32(buf, n - 4)
    # before the bloom section: a BlockMeta section of at least num | max_ts | crc, and meta_offset;
    # the bloom section [bo, n - 4) is at least k | crc
    if bo < 20 or bo + 5 > n - 4:
        return refused
    mo, sec_end = _u32(buf, bo - 4), bo - 4
    if mo + 16 > sec_end:
        return refused
    num = _u32(buf, mo)
    if num < 1 or num * kMetaRecMin + 16 > sec_end - mo:
        return refused
    err = 0
    if zlib.crc32(buf[mo + 4:sec_end - 4]) != _u32(buf, sec_end - 4) or zlib.crc32(buf[bo:n - 8]) != _u32(buf, n - 8):
        err |= ERR_CHECKSUM
    rec_end = sec_end - 12  # the records end where max_ts starts
    pos, index, ok = mo + 4, [], True
    first = last = None
    for i in range(num):
        if pos + 6 > rec_end:
            ok = False
            break
        off, fl = struct.unpack_from(">IH", buf, pos)
        kpos = pos + 6
        if kpos + fl + 8 + 2 > rec_end:
            ok = False
            break
        ll = struct.unpack_from(">H", buf, kpos + fl + 8)[0]
        lpos = kpos + fl + 10
        if lpos + ll + 8 > rec_end:
            ok = False
            break
        # a framed block holds at least its u16 entry count and its u32 CRC, inside the data section,
        # after the block before
        if off + 6 > mo or (index and off < index[-1]["off"] + 6):
            ok = False
            break
        hi, lo = image_ints(buf[kpos:kpos + fl])
        index.append(dict(img_hi=hi, img_lo=lo, off=off, end=mo, key_pos=kpos, key_len=fl))
        if i:
            index[-2]["end"] = off
        else:
            first = (kpos, fl)
        last = (lpos, ll)
        pos = lpos + ll + 8
    if ok and pos != rec_end:
        ok = False
    if not ok:
        err |= ERR_MALFORMED
    if err:
        return err, num, None, None
    desc = dict(nblk=num, meta_offset=mo, bloom_len=n - 4 - bo - 5, bloom_pos=bo, first_key_pos=first[0],
                first_key_len=first[1], last_key_pos=last[0], last_key_len=last[1],
                max_ts=int.from_bytes(buf[rec_end:rec_end + 8], "big"), bloom_k=buf[n - 9], err=0)
    return 0, num, desc, index


def open_batch_rule(files, file_off, index_cap=None):
    """The whole call over files[file_off[s]:file_off[s+1]] -> dict(desc, index, stats, reserved):
    desc[s] holds every field for an opened SST and only blk0 / nblk / err for a failed one; index is
    the list of all reserved slots, None where a slot belongs to a failed SST; stats = [SSTs opened,
    slots reserved, OR of the err, call-wide flags].  index_cap None: exactly what is required.
    Under a call-wide flag nothing is opened: desc and index are None."""
    nsst = len(file_off) - 1
    if any(b < a for a, b in zip(file_off, file_off[1:])):
        return dict(desc=None, index=None, stats=[0, None, None, ERR_MALFORMED], reserved=None)
    descs, index, blk0, opened, any_err = [], [], 0, 0, 0
    for s in range(nsst):
        fo = file_off[s]
        err, slots, d, recs = open_rule(files[fo:file_off[s + 1]])
        if err:
            descs.append(dict(blk0=blk0, nblk=0, err=err))
            index += [None] * slots
        else:
            d = dict(d, blk0=blk0)
            for f in ("bloom_pos", "first_key_pos", "last_key_pos"):
                d[f] += fo
            descs.append(d)
            index += recs
            opened += 1
        any_err |= err
        blk0 += slots
    if index_cap is not None and blk0 > index_cap:
        return dict(desc=None, index=None, stats=[0, blk0, None, ERR_CAPACITY], reserved=blk0)
    return dict(desc=descs, index=index, stats=[opened, blk0, any_err, 0], reserved=blk0)


# ------------------------------------------------------------------------------ the window classifier
Read = namedtuple("Read", "rec kind nb refill before first gap")


def _trace(buf, file_start):
    err, _, _, index = open_rule(buf)
    if index is None:
        return [], None
    out, wbase = [], None

    def read(rec, kind, p, nb):
        nonlocal wbase
        ap = file_start + p
        if wbase is None or ap < wbase or ap + nb > wbase + kOpenChunk:
            before = 0 if wbase is None else min(max(wbase + kOpenChunk - ap, 0), nb)
            gap = 0 if wbase is None else max(ap - (wbase + kOpenChunk), 0)
            out.append(Read(rec, kind, nb, True, before, wbase is None, gap))
            wbase = ap & ~15
        else:
            out.append(Read(rec, kind, nb, False, nb, False, 0))

    for i, r in enumerate(index):
        read(i, "header", r["key_pos"] - 6, 6)
        if r["key_len"]:
            read(i, "key", r["key_pos"], min(r["key_len"], IMG_BYTES))
        read(i, "length", r["key_pos"] + r["key_len"] + 8, 2)
    return out, wbase


def window_trace(buf, file_start):
    """The walk's field reads of a file that opens, in order -- a 6-byte header, min(fl, 16) bytes of
    the first key (none for an empty key), the 2-byte last-key length -- through a window of
    kOpenChunk bytes that is rebased to the field's absolute position rounded down to 16 whenever the
    field is not wholly inside it.  Per read: (rec, kind, nb, refill, before, first, gap) -- `before`
    = bytes of the field before the old window's end (nb without a refill), `first` = the file's
    first fill, `gap` = bytes between the old window's end and the field."""
    return _trace(buf, file_start)[0]


# ------------------------------------------------------------------------------ generators
KINDS = ("header", "key", "length")
FIELD_BYTES = {"header": 6, "key": IMG_BYTES, "length": 2}
# (split, first-key length of the straddling record): split = bytes of the field before the window's
# end; 0 = the field starts exactly at the end, all of them = it ends exactly there (no refill)
SPLITS = {"header": [(s, 3) for s in range(7)],
          "key": [(s, 20) for s in range(17)] + [(0, 1), (1, 1), (3, 7), (7, 7), (15, 16), (16, 16)],
          "length": [(s, 3) for s in range(3)]}
Straddle = namedtuple("Straddle", "kind split fl buf")


def _straddle_one(kind, split, fl, residue, rng):
    """Three records: record 1 has its `kind` field `split` bytes before the first window's end, the
    last record the same field at the complementary split before the end of the window after that.
    The fields are placed by the length of the record before's last key, which the walk never reads;
    the window in effect is asked of _trace over the records so far."""
    nb = min(fl, IMG_BYTES) if kind == "key" else FIELD_BYTES[kind]
    assert split <= nb
    data_len = 40
    pre = {"header": 0, "key": 6, "length": 6 + fl + 8}[kind]  # the field's place in its record
    key = lambda n: bytes(rng.integers(0, 256, n, dtype=np.uint8))
    f0 = key(5)
    p0 = data_len + 4
    end1 = p0 - (residue + p0) % 16 + kOpenChunk  # file-relative end of the window filled at p0
    l0 = end1 - split - pre - (p0 + 24 + len(f0))
    recs = [(0, f0, key(l0)), (6, key(fl), b"")]
    _, wbase = _trace(craft(recs, data_len=data_len), residue)
    if wbase + kOpenChunk - residue == end1:
        # record 1 ended with its window (the length's last byte is the window's): a short record
        # takes the refill, so that the record after it can meet the next window's end
        recs.append((12, key(4), b""))
        _, wbase = _trace(craft(recs, data_len=data_len), residue)
    h2 = data_len + 4 + sum(len(record(*r)) for r in recs)  # the last record's header, the one before's last key empty
    l1 = wbase + kOpenChunk - residue - (nb - split) - pre - h2
    recs[-1] = recs[-1][:2] + (key(l1),)
    recs.append((6 * len(recs), key(fl), key(9)))
    return craft16(recs, data_len=data_len, max_ts=(residue << 8) | split)


@lru_cache(maxsize=None)
def straddle_files(kind, residue):
    """Files of two to three windows of BlockMeta bytes, built for a file start at `residue` (mod
    16), every length a multiple of 16: one per entry of SPLITS[kind]."""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + residue)
    return [Straddle(kind, split, fl, _straddle_one(kind, split, fl, residue, rng)) for split, fl in SPLITS[kind]]


LONG_LENS = (kOpenChunk - 1, kOpenChunk, kOpenChunk + 1, 3 * kOpenChunk, 65535)
MASK_KEYS = ([b"fifteen-bytes-k"] + [b"sixteen-bytes-k" + b for b in (b"\x00", b"\xff")] +
             [b"seventeen-bytes" + a + b for a in (b"\x00", b"\xff") for b in (b"\x00", b"\xff")])


@lru_cache(maxsize=None)
def long_key_files():
    """[(label, file)], every length a multiple of 16: first and last keys of LONG_LENS (the field
    after a long key lies whole windows ahead), both keys at 65535, empty keys, and 15 / 16 / 17-byte
    keys whose 16th and 17th bytes and following ts bytes are 0x00 and 0xFF (the image's masking)."""
    rng = np.random.default_rng(77)
    key = lambda n: bytes(rng.integers(0, 256, n, dtype=np.uint8))
    out = []
    for n in LONG_LENS:
        out.append(("first-%d" % n, craft16([(0, b"a", b"b"), (8, key(n), b"c"), (16, b"d", b"e")], data_len=32)))
        out.append(("last-%d" % n, craft16([(0, b"a", key(n)), (8, b"bcd", b"c"), (16, key(n), key(n))], data_len=32)))
    out.append(("both-65535", craft16([(0, key(65535), key(65535)), (6, b"z", b"zz")], data_len=12)))
    out.append(("empty-first", craft16([(0, b"", b"b"), (8, b"c", b"d")], data_len=20)))
    out.append(("empty-last", craft16([(0, b"a", b"b"), (8, b"c", b"")], data_len=20)))
    out.append(("empty-all", craft16([(0, b"", b""), (6, b"", b""), (12, b"", b"")], data_len=18)))
    assert [len(k) for k in MASK_KEYS] == [15, 16, 16, 17, 17, 17, 17]
    mask = [(8 * i, k, k, ts, ts) for i, (k, ts) in enumerate((k, ts) for k in MASK_KEYS for ts in (0, ALL_ONES))]
    out.append(("image-mask", craft16(mask, data_len=8 * len(mask) + 8)))
    return out


Edge = namedtuple("Edge", "edge side buf")  # side: "accept" / "refuse" = the side of the check's boundary


def smallest_file():
    """59 bytes: a 6-byte data section, one record of empty keys, an empty filter."""
    return craft([(0, b"", b"")], data_len=6)


def _base_metas(nrec=3):
    return [(8 * i, b"first-%02d" % i, b"last-%02d-x" % i) for i in range(nrec)]


@lru_cache(maxsize=None)
def edge_files():
    """One file on each side of every bounds check of the open.  Where a side's file cannot be a
    whole valid SST (a BlockMeta section of exactly 16 bytes has no record), the file is still on
    that side of THAT check and fails a later one: the rule decides what is expected."""
    E, base = [], _base_metas()
    add = lambda edge, side, buf: E.append(Edge(edge, side, buf))
    # ---- prep: footers
    bare = dict(metas=[], data_len=0, num=1)  # num | max_ts | crc | meta_offset = 20 bytes, then the bloom section
    add("bloom_offset_low", "accept", craft(**bare))                       # bloom_offset == 20
    add("bloom_offset_low", "refuse", craft(**bare, bloom_offset=19))
    for bo in (0, 3, 4):
        add("bloom_offset_low", "refuse", craft(base, bloom_offset=bo))
    ok = craft(base)                                                       # an empty filter: bloom_offset == len - 9
    assert _u32(ok, len(ok) - 4) == len(ok) - 9
    add("bloom_offset_high", "accept", ok)
    add("bloom_offset_high", "refuse", craft(base, bloom_offset=len(ok) - 8))
    add("bloom_offset_high", "refuse", craft(base, bloom_offset=len(ok)))
    add("bloom_offset_high", "refuse", craft(base, bloom_offset=0xFFFFFFFF))
    add("meta_offset_high", "accept", craft([], data_len=10, num=1))       # meta_offset + 16 == bloom_offset - 4
    add("meta_offset_high", "refuse", craft([], data_len=10, num=1, meta_offset=11))
    add("meta_offset_high", "refuse", craft(base, meta_offset=0xFFFFFFF0))
    # ---- prep: the count
    add("num_low", "accept", craft(base[:1]))
    add("num_low", "refuse", craft(base[:1], num=0))
    empty = [(6 * i, b"", b"") for i in range(5)]                          # num * kMetaRecMin + 16 == the section
    add("num_section", "accept", craft(empty))
    add("num_section", "refuse", craft(empty, num=6))
    add("num_section", "refuse", craft(base, num=0xFFFFFFFF))
    add("num_section", "refuse", craft(base, num=0xAAAAAAAB))              # * 24 wraps to 8 in 32 bits
    # ---- walk: offsets
    two = lambda o1: [(0, b"k0", b"k1"), (o1, b"k2", b"k3")]
    add("offset_step", "accept", craft(two(6)))
    add("offset_step", "refuse", craft(two(5)))
    add("offset_step", "refuse", craft(two(0)))
    add("offset_step", "accept", craft([(10, b"k0", b"k1"), (16, b"k2", b"k3"), (22, b"k4", b"k5")]))
    add("offset_step", "refuse", craft([(10, b"k0", b"k1"), (16, b"k2", b"k3"), (21, b"k4", b"k5")]))
    add("offset_last", "accept", craft(two(64 - 6)))                       # data_len 64 = meta_offset
    add("offset_last", "refuse", craft(two(64 - 5)))
    add("offset_last", "refuse", craft(two(0xFFFFFFFF)))
    add("offset_last", "accept", craft([(58, b"only", b"one")]))
    add("offset_last", "refuse", craft([(59, b"only", b"one")]))
    add("offset_first", "accept", craft([(17, b"k0", b"k1"), (30, b"k2", b"k3")]))  # a nonzero first offset opens
    add("offset_first", "refuse", craft([(0xFFFFFFFA, b"k0", b"k1")]))              # ... inside the data section
    # ---- walk: the records' end
    add("records_end", "accept", craft(base))
    add("records_end", "refuse", craft(base, pad=b"\0"))                   # one byte too many
    add("records_end", "refuse", craft(base[:2] + [record(*base[2])[:-1]]))  # one too few
    long3 = [(8 * i, b"a-first-key-of-20-by" + bytes([i]), b"a-last-key-of-20-byt" + bytes([i])) for i in range(3)]
    add("count_present", "accept", craft(long3))
    add("count_present", "refuse", craft(long3, num=4))                    # passes the count check: 4 * 24 + 16 <= the section
    add("count_present", "refuse", craft(long3, num=2))
    for n in (1, 5, 6, 7):                                                 # a header past the end by 5 and by 1; one that fits
        add("header_end", "refuse", craft(long3, num=4, pad=bytes(n)))
    add("header_end", "accept", craft(long3 + [(24, b"", b"")]))           # the same count with its record present
    # the last record, 46 bytes, claims a first key / last key that runs past the records' end by one byte
    claim = lambda ll: struct.pack(">IH", 24, 20) + bytes(28) + struct.pack(">H", ll) + bytes(10)
    add("first_key_end", "refuse", craft(long3 + [struct.pack(">IH", 24, 31) + bytes(40)]))  # 6 + 31 + 10 == 47
    add("first_key_end", "accept", craft(long3 + [record(24, bytes(20), bytes(2))]))
    add("last_key_end", "refuse", craft(long3 + [claim(3)]))               # 6 + 20 + 10 + 3 + 8 == 47
    add("last_key_end", "accept", craft(long3 + [claim(2)]))
    # ---- every length below the smallest valid file
    small = smallest_file()
    assert len(small) == 59
    add("file_length", "accept", small)
    for n in range(59):
        for fill in (bytes(n), b"\xff" * n, small[59 - n:]):
            add("file_length", "refuse", fill)
    return E


EDGES = ("bloom_offset_low", "bloom_offset_high", "meta_offset_high", "num_low", "num_section", "offset_step",
         "offset_last", "offset_first", "records_end", "count_present", "header_end", "first_key_end", "last_key_end",
         "file_length")
# checks whose two sides no output can tell apart: a BlockMeta section that these footers leave is too
# short for one record, so the accepted side fails the count check, with no slot reserved either
SAME_BOTH_SIDES = ("bloom_offset_low", "meta_offset_high")


def _flip(buf, pos, bit=0):
    b = bytearray(buf)
    b[pos] ^= 1 << bit
    return bytes(b)


@lru_cache(maxsize=None)
def crc_files():
    """[(label, file, expected err)]: one bit flipped per place a section CRC covers or is, a flip in
    the data section (which still opens: block CRCs are not the open's job), and two files that are
    CHECKSUM | MALFORMED."""
    metas = _base_metas(4)
    buf = craft(metas, max_ts=0x0102030405060708, bloom=(junk(24, 5), 6), data_len=48)
    n = len(buf)
    bo = _u32(buf, n - 4)
    mo = _u32(buf, bo - 4)
    out = [("intact", buf, 0),
           ("record-byte", _flip(buf, mo + 4 + 6 + 2, 3), ERR_CHECKSUM),   # a first-key byte
           ("record-offset", _flip(buf, mo + 4 + 3, 1), ERR_CHECKSUM),     # 0 -> 2: still increasing
           ("max-ts", _flip(buf, bo - 16 + 7), ERR_CHECKSUM),
           ("meta-crc", _flip(buf, bo - 8, 7), ERR_CHECKSUM),
           ("filter-byte", _flip(buf, bo + 11, 4), ERR_CHECKSUM),
           ("k-byte", _flip(buf, n - 9, 2), ERR_CHECKSUM),
           ("bloom-crc", _flip(buf, n - 5), ERR_CHECKSUM),
           ("data-section", _flip(buf, 20, 6), 0),
           # a first-key length's high byte: the meta CRC fails and the key runs past the records' end
           ("key-length-byte", _flip(buf, mo + 4 + 4, 6), ERR_CHECKSUM | ERR_MALFORMED),
           # a filter bit, and one byte too many after the last record under a correct meta CRC
           ("filter-and-tail", _flip(craft(metas, bloom=(junk(24, 5), 6), data_len=48, pad=b"\x01"), bo + 1 + 3), ERR_CHECKSUM | ERR_MALFORMED)]
    return out


def healthy(i):
    """A small file that opens, 1..4 records, different for every i."""
    nrec = 1 + i % 4
    return craft([(7 * j, b"h%d-f%d" % (i, j) * (1 + i % 3), b"h%d-l%d" % (i, j)) for j in range(nrec)], max_ts=1000 + i,
                 bloom=(junk(i % 9, i), 1 + i % 30), data_len=40 + i % 16)


def walk_failed(i=0):
    """Fails in the walk: its claimed slots stay reserved."""
    return (craft(_base_metas(3), pad=b"\0"), craft(_base_metas(2), meta_crc=5),
            craft([(0, b"a", b"b"), (5, b"c", b"d")]))[i % 3]


def prep_refused(i=0):
    """Refused by its footers or count: no slot reserved."""
    return (craft(_base_metas(3), num=0), craft(_base_metas(3), bloom_offset=7), bytes(30))[i % 3]


Batch = namedtuple("Batch", "name bufs start file_off")  # file_off None: back to back from `start`


def _batch(name, bufs, start=0, file_off=None):
    return Batch(name, list(bufs), start, file_off)


@lru_cache(maxsize=None)
def batches():
    B = [_batch("one-healthy", [healthy(0)], 5), _batch("one-walk-failed", [walk_failed(0)]),
         _batch("one-prep-refused", [prep_refused(0)], 16),
         _batch("two-failed-first", [walk_failed(1), healthy(1)], 3), _batch("two-refused-last", [healthy(2), prep_refused(1)])]
    b65 = [healthy(i) for i in range(65)]
    b65[0], b65[1], b65[32], b65[64] = walk_failed(0), prep_refused(0), prep_refused(1), walk_failed(2)
    B.append(_batch("65-mixed", b65, 9))
    b130 = [healthy(i + 3) for i in range(130)]
    b130[0], b130[64], b130[65], b130[100], b130[129] = prep_refused(2), walk_failed(1), walk_failed(0), b"", prep_refused(0)
    B.append(_batch("130-mixed", b130, 0))
    b3 = [healthy(7), healthy(8), healthy(9)]
    n = [len(b) for b in b3]
    B.append(_batch("decreasing", b3, 0, [0, n[0] + n[1], n[0], n[0] + n[1] + n[2]]))
    return B


def batch_layout(b):
    """(files bytes with `start` junk bytes in front, file_off)."""
    blob = junk(b.start, 201) + b"".join(b.bufs)
    if b.file_off is not None:
        return blob, list(b.file_off)
    off = [b.start]
    for x in b.bufs:
        off.append(off[-1] + len(x))
    return blob, off


def batch_shape(b):
    """What makes a batch a case: its size and where its failures of each kind stand."""
    blob, off = batch_layout(b)
    if any(y < x for x, y in zip(off, off[1:])):
        return dict(n=len(b.bufs), decreasing=True)
    rule = [open_rule(x) for x in b.bufs]
    kind = ["ok" if not r[0] else "reserved" if r[1] else "none" for r in rule]
    n = len(kind)
    where = lambda k: {("first" if i == 0 else "last" if i == n - 1 else "middle") for i, x in enumerate(kind) if x == k and n > 1}
    return dict(n=n, decreasing=False, reserved=where("reserved"), none=where("none"),
                neighbours=sum(a != "ok" and c != "ok" for a, c in zip(kind, kind[1:])),
                zero_between=sum(len(b.bufs[i]) == 0 and kind[i - 1] == "ok" == kind[i + 1] for i in range(1, n - 1)))
