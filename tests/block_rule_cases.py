"""Blocks that break each block-validation rule by the least amount -- TEST INFRASTRUCTURE.

The rules ("Validation rules"; parse_hdr / parse_entry in lsmblk_dev.hpp, restated by
seek_kernel in lsmblk_sst.hip and by the oracle's decode):

  len         len >= 2
  count       2 + 2n <= len
  data_end    data_end >= 4                      (n > 0)
  first_key   4 + fks + 8 <= data_end            (n > 0)
  offset      off + 4 <= data_end                per entry
  suffix_len  off + 4 + s + 10 <= data_end
  prefix      p <= fks
  empty_key   p + s > 0
  value_len   off + 14 + s + vl <= data_end

Two base blocks from oracle.Builder: `small` (5 entries, read through the kernels' LDS images) and
`big` (70 entries, larger than both staging limits, read through buffer descriptors).  In both,
entry 1's key is the first key plus one byte (p == fks, the valid side of `prefix`) and the last
entry has an empty value and ends at data_end (the valid side of the two length rules).  Every
variant is a base block with one field rewritten; `len` and `data_end` are raw blocks of their own.
Shared by test_block_rule_cases.py (CPU: the oracle's verdicts) and test_gpu_block_rules.py (GPU:
every consumer gives that verdict).
"""
import os
from dataclasses import dataclass
from functools import lru_cache

import path_cases as pc
from oracle import oracle as O

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsm_amd", "csrc")
kGetLdsBlock = pc.read_constants(os.path.join(_CSRC, "lsmblk_get.hip"), ("kGetLdsBlock",))["kGetLdsBlock"]
STAGING_LIMIT = max(kGetLdsBlock, pc.kDecImg, 5120)  # a block above it is staged by no kernel

RULES = ("len", "count", "data_end", "first_key", "offset", "suffix_len", "prefix", "empty_key", "value_len")
RAW_RULES = ("len", "data_end")  # raw blocks, for the decode alone
SIZES = ("small", "big")
BROKEN = {"small": 5 // 2, "big": 67}  # seek_kernel's first probe; a lane of the second round of 64


@dataclass
class Case:
    name: str
    size: str          # "small" / "big" / "raw"
    rule: str          # the rule it breaks; None: a base block
    block: bytes
    seek_key: bytes    # the key the seek and the point read look up; None: decode only
    broken: int        # the entry the variant rewrites; None: the header (or a base block)


def base_entries(size):
    n, vlen = (5, 3) if size == "small" else (70, 80)
    keys = [b"key-00", b"key-00a"] + [b"key-%02d" % i for i in range(2, n)]
    return [(k, 1000 + i, b"" if i == n - 1 else bytes([65 + i % 26]) * vlen) for i, k in enumerate(keys)]


@lru_cache(maxsize=None)
def base_block(size):
    b = O.Builder(1 << 15)
    for k, ts, v in base_entries(size):
        assert b.add(k, ts, v)
    return b.finish()


def u16(buf, i):
    return int.from_bytes(buf[i:i + 2], "big")


def layout(blk):
    """(n, data_end, fks, entry offsets) of a well-formed block."""
    n = u16(blk, len(blk) - 2)
    data_end = len(blk) - 2 - 2 * n
    return n, data_end, u16(blk, 2), [u16(blk, data_end + 2 * i) for i in range(n)]


def seek_path(n, target):
    """BlockIterator::seek_to_key's probes (mid = lo + (hi - lo) / 2) on the way to entry `target`."""
    lo, hi, path = 0, n, []
    while lo < hi:
        mid = lo + (hi - lo) // 2
        path.append(mid)
        if mid < target:
            lo = mid + 1
        elif mid > target:
            hi = mid
        else:
            break
    return path


def _put(blk, at, value):
    out = bytearray(blk)
    out[at:at + 2] = value.to_bytes(2, "big")
    return bytes(out)


def variants(size):
    blk = base_block(size)
    ents = base_entries(size)
    n, data_end, fks, offs = layout(blk)
    k, last = BROKEN[size], n - 1
    s_last = u16(blk, offs[last] + 2)
    assert offs[last] + 14 + s_last == data_end  # the empty value: the last entry ends at data_end
    mk = lambda rule, block, broken: Case(f"{size}-{rule}", size, rule, block, ents[k if broken is None else broken][0], broken)
    return [
        mk("count", _put(blk, len(blk) - 2, (len(blk) - 2) // 2 + 1), None),
        mk("first_key", _put(blk, 2, data_end - 11), None),
        mk("offset", _put(blk, data_end + 2 * k, data_end - 3), k),
        mk("suffix_len", _put(blk, offs[last] + 2, s_last + 1), last),
        mk("prefix", _put(blk, offs[k], fks + 1), k),
        mk("empty_key", _put(_put(blk, offs[k], 0), offs[k] + 2, 0), k),
        mk("value_len", _put(blk, offs[last] + 12 + s_last, 1), last),
    ]


@lru_cache(maxsize=None)
def cases():
    out = []
    for size in SIZES:
        out.append(Case(f"{size}-base", size, None, base_block(size), base_entries(size)[BROKEN[size]][0], None))
        out += variants(size)
    out.append(Case("raw-len", "raw", "len", b"\x00", None, None))
    out.append(Case("raw-data_end", "raw", "data_end", b"\x00\x00\x00" + b"\x00\x00" + b"\x00\x01", None, None))
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


NAMES = [c.name for c in cases()]


@lru_cache(maxsize=None)
def verdict(name):
    """The oracle's decode of the case's block -> (rc, entries or None)."""
    import numpy as np
    c = case(name)
    rc, kv = O.decode_blocks(np.frombuffer(c.block, np.uint8), np.array([0, len(c.block)], np.uint64))
    return rc, (kv.entries() if rc == O.ORC_OK else None)


# ------------------------------------------------------------------------------ the block inside an SST
OTHER_ENTRIES = [(b"other-%02d" % i, 500 + i, b"v%02d" % i) for i in range(12)]


@lru_cache(maxsize=None)
def sst_pair(size):
    """(files, file_off, position of the base block in files): table 0 holds the base block's
    entries as its one block, table 1 other keys."""
    from oracle import pyref
    f0 = pyref.sst_file(base_entries(size), 1 << 15)
    f1 = pyref.sst_file(OTHER_ENTRIES, 64)
    metas, _, _, meta_offset = pyref.sst_open(f0)
    assert len(metas) == 1 and f0[metas[0][0]:meta_offset - 4] == base_block(size)
    return f0 + f1, [0, len(f0), len(f0) + len(f1)], metas[0][0]
