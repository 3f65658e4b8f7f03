"""GPU parity of the decode's in-place value compaction (dec_fast_outputs: the chunk map, the
ascending moves inside the staged block, the edge chunks from registers, the key image) and of its
fallbacks: the batches of tests/decode_inplace_cases.py, whose routes test_decode_inplace_cases.py
asserts on the CPU and this file again under the tensors' real addresses.

Every batch goes through the lagged and the two-pass decode.  Keys, key_off, values, val_off, ts
(and the block entry index) and the status words are compared with the C oracle's decode bit for
bit; the outputs are prefilled tensors whose capacities are exactly the totals, and every byte
before the arrays and past the totals must still hold the prefill.
"""
import numpy as np
import pytest
import torch

import decode_cases as dc
import decode_inplace_cases as ic
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch
from lsm_amd._lib import lib
from oracle import oracle as O
from test_gpu_decode_routes import TWO_PASS, decode_exact, place

pytestmark = pytest.mark.gpu

MODES = ("default", "two_pass")


@pytest.fixture(scope="module")
def cases():
    """name -> (batch, the oracle's KV, block entry index), built once and read-only."""
    memo = {}

    def get(name):
        if name not in memo:
            b = ic.CASES[name]()
            rc, kv = O.decode_blocks(b.blocks, b.blk_off)
            assert rc == 0
            ent = np.cumsum([0] + [dc.parse(x)[0] for x in b.bufs]).astype(np.int64)
            for a in (kv.keys, kv.key_off, kv.vals, kv.val_off, kv.ts, ent):
                a.flags.writeable = False
            memo[name] = (b, kv, ent)
        return memo[name]
    return get


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", tuple(ic.CASES))
def test_decode_inplace(cases, name, mode):
    b, kv, ent = cases(name)
    nblk = len(b.bufs)
    do = torch.from_numpy(np.ascontiguousarray(b.blk_off, np.uint64).view(np.int64)).cuda()
    db = place(b.blocks, 0)
    # the routes under the tensor's real address are the ones the CPU test asserted at address 0
    assert db.data_ptr() % 16 == 0
    want = [r for _, r, _ in ic.routes(b)]
    assert [r for _, r, _ in ic.routes(b, base=db.data_ptr())] == want
    assert "inplace" in want
    ctx = batch._ctx(0)
    try:
        assert lib().lsmblk_debug_set(ctx, TWO_PASS, int(mode == "two_pass")) == 0
        decode_exact(db, do, nblk, kv, ent, mode)
    finally:
        lib().lsmblk_debug_set(ctx, TWO_PASS, 0)
