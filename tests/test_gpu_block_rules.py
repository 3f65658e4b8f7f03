"""Every consumer of a block gives the oracle's verdict on every block-validation rule
(block_rule_cases.py): the decode (lagged, two-pass, and the verifying decode's count in the CRC
pass), seek_kernel, and -- the block overwritten inside an opened SST, so that the read kernels
judge it and not the open -- the point read and the range scan.  A refused block is reported the
way each call's own malformed test expects; the base blocks give the oracle's entries."""
import zlib

import numpy as np
import pytest
import torch

import block_rule_cases as brc
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch, sst
from lsm_amd._lib import LSMBLK_DEBUG_TWO_PASS_DECODE, LSMBLK_ERR_MALFORMED, LSMBLK_E_MALFORMED, LsmBlkError, lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GET_ABSENT, GET_FOUND, GET_TOMBSTONE = 0, 1, 2
SCAN_OK, SCAN_EMPTY = 0, 1
NO_FILTER, MVCC = 1, 2
CAPS = (256, 4096, 16384)
SST_NAMES = [c.name for c in brc.cases() if c.size != "raw"]


def dev_block(block, tail=b""):
    data = bytes(block) + tail
    buf = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
    buf[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return buf[:len(data)], torch.tensor([0, len(data)], dtype=torch.int64, device="cuda")


def entries_of(kv):
    keys, ko, vals, vo, ts = kv.to_numpy()
    return [(keys[ko[i]:ko[i + 1]].tobytes(), int(ts[i]), vals[vo[i]:vo[i + 1]].tobytes()) for i in range(kv.n)]


def check_decode(name, **kw):
    c = brc.case(name)
    rc, ents = brc.verdict(name)
    tail = zlib.crc32(c.block).to_bytes(4, "big") if kw.get("verify") else b""  # the CRC of the bytes as they are
    db, do = dev_block(c.block, tail)
    if rc == O.ORC_OK:
        assert entries_of(batch.decode_blocks(db, do, **kw)) == ents
    else:
        with pytest.raises(LsmBlkError) as e:
            batch.decode_blocks(db, do, **kw)
        assert e.value.status == LSMBLK_E_MALFORMED


@pytest.mark.parametrize("name", brc.NAMES)
def test_decode(name):
    check_decode(name)


@pytest.mark.parametrize("name", brc.NAMES)
def test_two_pass_decode(name):
    ctx = batch._ctx(0)
    assert lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_TWO_PASS_DECODE, 1) == 0
    try:
        check_decode(name)
    finally:
        lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_TWO_PASS_DECODE, 0)


@pytest.mark.parametrize("name", brc.NAMES)
def test_verifying_decode(name):
    check_decode(name, tail=4, verify=True)


@pytest.mark.parametrize("name", brc.NAMES)
def test_two_pass_verifying_decode(name):
    """crc_kernel<true>'s count_block, the fused count of the two-pass verifying decode."""
    ctx = batch._ctx(0)
    assert lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_TWO_PASS_DECODE, 1) == 0
    try:
        check_decode(name, tail=4, verify=True)
    finally:
        lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_TWO_PASS_DECODE, 0)


@pytest.mark.parametrize("name", SST_NAMES)
def test_seek(name):
    c = brc.case(name)
    rc, _ = brc.verdict(name)
    db, do = dev_block(c.block)
    if rc == O.ORC_OK:
        keys = [k for k, _, _ in brc.base_entries(c.size)]
        want = [O.seek_key(c.block, k) for k in keys]
        assert batch.seek_blocks(db, do, [0] * len(keys), keys).tolist() == want == list(range(len(keys)))
    else:
        with pytest.raises(LsmBlkError) as e:
            batch.seek_blocks(db, do, [0], [c.seek_key])
        assert e.value.status == LSMBLK_E_MALFORMED


# ------------------------------------------------------------------------------ the block inside an SST
_sets = {}
OTHER_KEYS = [k for k, _, _ in brc.OTHER_ENTRIES]


def other_reads(ss):
    """Table 1's point reads and its range, as (get results, scan result, scanned entries)."""
    g, _, _, gst = ss.get_raw([1] * len(OTHER_KEYS), OTHER_KEYS, 1 << 40, NO_FILTER)
    return g


def opened(size):
    if size not in _sets:
        files, file_off, pos = brc.sst_pair(size)
        ss = sst.SstSet(files, file_off)
        assert ss.err.tolist() == [0, 0]
        _sets[size] = (ss, pos, other_reads(ss).copy())
    return _sets[size]


class victim_block:
    """The case's block in place of the base block in the opened set's device bytes."""

    def __init__(self, ss, pos, c):
        self.ss, self.pos, self.c = ss, pos, c

    def put(self, block):
        self.ss.files[self.pos:self.pos + len(block)] = torch.frombuffer(bytearray(block), dtype=torch.uint8).to(self.ss.device)
        torch.cuda.synchronize(self.ss.device)

    def __enter__(self):
        self.put(self.c.block)

    def __exit__(self, *exc):
        self.put(brc.base_block(self.c.size))


@pytest.mark.parametrize("name", SST_NAMES)
def test_sst_get(name):
    c = brc.case(name)
    rc, ents = brc.verdict(name)
    ss, pos, others = opened(c.size)
    with victim_block(ss, pos, c):
        if rc == O.ORC_OK:
            g = ss.get([0] * len(ents), [k for k, _, _ in ents], 1 << 40, no_filter=True)
            assert g["status"].tolist() == [GET_FOUND if v else GET_TOMBSTONE for _, _, v in ents]
            assert g["ts"].tolist() == [ts for _, ts, _ in ents]
            assert g["hit_ent"].tolist() == list(range(len(ents)))
            assert g["values"] == [v or None for _, _, v in ents]
        else:
            r, _, _, st = ss.get_raw([0] + [1] * len(OTHER_KEYS), [c.seek_key] + OTHER_KEYS, 1 << 40, NO_FILTER)
            assert st[3] == LSMBLK_ERR_MALFORMED
            assert r["status"][0] == GET_ABSENT and r["vlen"][0] == 0
            assert r[1:].tobytes() == others.tobytes()  # the other table's keys: answered as before


@pytest.mark.parametrize("name", SST_NAMES)
def test_sst_scan(name):
    c = brc.case(name)
    rc, ents = brc.verdict(name)
    ss, pos, _ = opened(c.size)
    base = brc.base_entries(c.size)
    lower, upper = [base[0][0], OTHER_KEYS[0]], [base[-1][0], OTHER_KEYS[-1]]
    with victim_block(ss, pos, c):
        r, seg, kv, st = ss.scan_raw([0, 1], lower, upper, "included", "included", NO_FILTER | MVCC, CAPS)
    got = entries_of(kv)
    if rc == O.ORC_OK:
        assert st[3] == 0 and r["status"].tolist() == [SCAN_OK, SCAN_OK]
        assert r["n"].tolist() == [len(ents), len(brc.OTHER_ENTRIES)] and seg.tolist() == [0, len(ents), len(got)]
        assert got == ents + brc.OTHER_ENTRIES
    else:
        assert st[3] == LSMBLK_ERR_MALFORMED
        assert r["status"].tolist() == [SCAN_EMPTY, SCAN_OK] and r["n"].tolist() == [0, len(brc.OTHER_ENTRIES)]
        assert seg.tolist() == [0, 0, len(brc.OTHER_ENTRIES)]
        assert got == brc.OTHER_ENTRIES  # the other table's range: answered as before
