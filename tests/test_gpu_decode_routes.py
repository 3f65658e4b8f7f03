"""GPU parity on the entry routes inside a block of the decode (dec_entry_runs and its sinks,
flush_chunks, dec_big_entry, copy_run, copy_long_runs, dec_simple_outputs): the batches of
tests/decode_cases.py (their coverage is asserted on the CPU by test_decode_cases.py, and again
here for the tensors' real addresses) through lsmblk_decode_batch at the default lag and at lag
128, the two-pass decode, and the framed, CRC-verifying read in both decode modes, the block stream
at address 0, 1, 8 and 15 mod 16 (the key shapes at all 16).

Every output is compared with the C oracle and with pyref.block_entries: n, key_off, val_off
(sentinels included), ts, keys, values and the block entry index.  The outputs are tensors
prefilled with a constant, the capacities exactly the totals: every byte and word before the
arrays and past the totals must still hold the constant.
"""
import numpy as np
import pytest
import torch

import decode_cases as dc
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch
from lsm_amd._lib import LSMBLK_DEBUG_DECODE_LAG, LSMBLK_DEBUG_TWO_PASS_DECODE, lib
from oracle import oracle as O
from test_gpu_parity import assert_kv_equal, framed_want

pytestmark = pytest.mark.gpu

MODES = ("default", "lag128", "two_pass", "framed_lagged", "framed_two_pass")
GUARD = 64  # prefilled bytes before and after every output array
TWO_PASS, LAG = LSMBLK_DEBUG_TWO_PASS_DECODE, LSMBLK_DEBUG_DECODE_LAG


@pytest.fixture(scope="module")
def cases():
    """name -> (batch, oracle KV, block entry index, framed bytes, framed offsets), built once."""
    memo = {}

    def get(name):
        if name not in memo:
            b = dc.GENERATORS[name]()
            rc, kv = O.decode_blocks(b.blocks, b.blk_off)
            assert rc == 0
            ref = O.KV.from_entries(b.entries())  # pyref's reading of the same blocks
            assert kv.n == ref.n
            for x, y in ((kv.key_off, ref.key_off), (kv.val_off, ref.val_off), (kv.ts, ref.ts), (kv.keys, ref.keys),
                         (kv.vals, ref.vals)):
                np.testing.assert_array_equal(x, y)
            ent = np.cumsum([0] + [dc.parse(x)[0] for x in b.bufs]).astype(np.int64)
            data, foff = framed_want(b.blocks, b.blk_off)
            for a in (kv.keys, kv.key_off, kv.vals, kv.val_off, kv.ts, ent):
                a.flags.writeable = False
            memo[name] = (b, kv, ent, np.frombuffer(data, np.uint8), foff)
        return memo[name]
    return get


def place(stream, shift):
    """The stream at an address that is `shift` mod 16, between GAP bytes."""
    buf = torch.full((len(stream) + shift + 32,), dc.GAP, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + len(stream)] = torch.from_numpy(np.array(stream, np.uint8))
    return buf[shift:shift + len(stream)]


def guarded(nbytes):
    """A prefilled byte buffer of GUARD + nbytes + GUARD (+ up to 15) bytes."""
    return torch.full((2 * GUARD + (nbytes + 15) // 16 * 16,), dc.FILL, dtype=torch.uint8, device="cuda")


def check_guarded(buf, want, what):
    """buf = GUARD prefill bytes, then exactly the bytes of `want`, then prefill to the end."""
    got = buf.cpu().numpy()
    w = np.ascontiguousarray(want).view(np.uint8).ravel()
    assert (got[:GUARD] == dc.FILL).all(), f"{what}: a write before the array"
    body = got[GUARD:GUARD + len(w)]
    if not np.array_equal(body, w):
        bad = np.flatnonzero(body != w)
        pytest.fail(f"{what}: {len(bad)} bytes differ, first at {bad[:8]} of {len(w)}")
    past = np.flatnonzero(got[GUARD + len(w):] != dc.FILL)
    assert past.size == 0, f"{what}: a write past the totals, at +{past[:8]}"


def decode_exact(db, do, nblk, kv, ent, mode):
    """One decode into prefilled outputs whose capacities are exactly the totals; every output and
    its surroundings against the oracle's."""
    n, K, V = kv.n, int(kv.key_off[-1]), int(kv.val_off[-1])
    bufs = {"keys": guarded(K), "key_off": guarded(4 * (n + 1)), "vals": guarded(V), "val_off": guarded(4 * (n + 1)),
            "ts": guarded(8 * n), "blk_ent": guarded(8 * (nblk + 1))}
    out = batch.KVStream(bufs["keys"][GUARD:], bufs["key_off"][GUARD:].view(torch.int32), bufs["vals"][GUARD:],
                         bufs["val_off"][GUARD:].view(torch.int32), bufs["ts"][GUARD:].view(torch.int64), 0)
    stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device="cuda")
    if mode == "default":
        batch.decode_into(db, do, nblk, out, stats, n, K, V)
        blk_ent = None
    else:
        blk_ent = bufs["blk_ent"][GUARD:].view(torch.int64)
        framed = mode.startswith("framed")
        batch.decode_ex_into(db, do, nblk, out, stats, n, K, V, tail=4 if framed else 0, verify=framed, blk_ent=blk_ent)
    torch.cuda.synchronize()
    assert batch._status(stats) == 0, mode
    assert stats[:3].cpu().tolist() == [n, K, V], mode
    check_guarded(bufs["key_off"], kv.key_off[:n + 1].astype(np.uint32), mode + " key_off")
    check_guarded(bufs["val_off"], kv.val_off[:n + 1].astype(np.uint32), mode + " val_off")
    check_guarded(bufs["ts"], kv.ts.astype(np.uint64), mode + " ts")
    check_guarded(bufs["keys"], kv.keys[:K], mode + " keys")
    check_guarded(bufs["vals"], kv.vals[:V], mode + " vals")
    check_guarded(bufs["blk_ent"], ent if blk_ent is not None else np.zeros(0, np.uint8), mode + " blk_ent")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", tuple(dc.GENERATORS))
def test_decode_routes(cases, name, mode):
    b, kv, ent, fdata, foff = cases(name)
    nblk = len(b.bufs)
    framed = mode.startswith("framed")
    stream, off = (fdata, foff) if framed else (b.blocks, b.blk_off)
    do = torch.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64)).cuda()
    ctx = batch._ctx(0)
    try:
        assert lib().lsmblk_debug_set(ctx, TWO_PASS, int(mode.endswith("two_pass"))) == 0
        assert lib().lsmblk_debug_set(ctx, LAG, 128 if mode == "lag128" else 0) == 0
        for ld in dc.GEN_LEADS[name]:
            db = place(stream, ld)
            decode_exact(db, do, nblk, kv, ent, mode)
            if mode == "default" and ld == 0:
                # the coverage under the tensor's real address
                miss, ev = dc.check(name, b, base=db.data_ptr())
                print(dc.coverage_line(name, b, ev))
                assert not miss, miss[:20]
    finally:
        lib().lsmblk_debug_set(ctx, TWO_PASS, 0)
        lib().lsmblk_debug_set(ctx, LAG, 0)


def test_amplified_blocks_take_the_capacity_retry(cases):
    """decode_blocks sizes its first output from the input bytes; the amplified blocks decode to
    several times that, so the first call reports CAPACITY with the needed sizes and the second
    one fits."""
    b, kv, ent, _, _ = cases("amplified")
    assert b.K > b.size + 16
    for ld in dc.LEADS:
        db = place(b.blocks, ld)
        do = torch.from_numpy(b.blk_off.view(np.int64)).cuda()
        got, gent = batch.decode_blocks(db, do, with_blk_ent=True)
        assert_kv_equal(got, kv)
        np.testing.assert_array_equal(gent.cpu().numpy(), ent)
