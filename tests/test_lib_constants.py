"""The ABI's numbers in lsm_amd/_lib.py against include/lsmblk.h and against ABI version 1 itself: the
tests and tools take the stats flags and the debug keys from _lib by name, so _lib is pinned here."""
import os
import re

from lsm_amd import _lib

with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lsmblk.h")) as _f:
    _H = _f.read()
HEADER = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (LSMBLK_\w+)[ \t]+(-?\d+)u?\b", _H, re.M)}

# ABI version 1, restated: renumbering the header and _lib together still fails here
ABI_1 = dict(
    LSMBLK_ERR_MALFORMED=1, LSMBLK_ERR_CAPACITY=2, LSMBLK_ERR_OVERFLOW=4, LSMBLK_ERR_TIMEOUT=8, LSMBLK_ERR_SEGMENTS=16,
    LSMBLK_ERR_INTERNAL=32, LSMBLK_ERR_EMPTY_KEY=64, LSMBLK_ERR_CHECKSUM=128,
    LSMBLK_DEBUG_POLL_MODE=0, LSMBLK_DEBUG_DECODE_SKIP=1, LSMBLK_DEBUG_KERNEL_TIMING=2, LSMBLK_DEBUG_TWO_PASS_DECODE=3,
    LSMBLK_DEBUG_DECODE_LAG=4, LSMBLK_DEBUG_COUNTERS=5, LSMBLK_DEBUG_DECODE_LAG_BYTES=6, LSMBLK_DEBUG_ROT_POISON=7,
    LSMBLK_DEBUG_ENCODE_FUSED=8, LSMBLK_DEBUG_PLAN_PIPE=9, LSMBLK_DEBUG_EMIT_POISON=10, LSMBLK_DEBUG_SCAN_UNITS=11,
    LSMBLK_DEBUG_EMIT_MODE=12)


def _is_flag_or_key(name):
    return name.startswith(("LSMBLK_ERR_", "LSMBLK_DEBUG_"))


def test_the_header_is_parsed():
    assert HEADER["LSMBLK_STATS_WORDS"] == 4 and HEADER["LSMBLK_LSM_SCAN_STATS_WORDS"] == 8
    assert sum(_is_flag_or_key(n) for n in HEADER) == 8 + 13


def test_every_define_of_the_header_that_lib_restates_has_the_headers_value():
    shared = [n for n in HEADER if hasattr(_lib, n)]
    assert len(shared) >= 40
    assert {n: getattr(_lib, n) for n in shared} == {n: HEADER[n] for n in shared}


def test_every_flag_and_debug_key_of_the_header_is_in_lib():
    assert [n for n in HEADER if _is_flag_or_key(n) and not hasattr(_lib, n)] == []


def test_flags_and_debug_keys_are_abi_version_1s():
    assert {n: getattr(_lib, n) for n in vars(_lib) if _is_flag_or_key(n)} == ABI_1
    assert sorted(v for n, v in ABI_1.items() if n.startswith("LSMBLK_DEBUG_")) == list(range(13))
    assert sorted(v for n, v in ABI_1.items() if n.startswith("LSMBLK_ERR_")) == [1 << i for i in range(8)]
