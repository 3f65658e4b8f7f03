"""The one-workgroup scans that end the batched calls (share1024 / block_excl1024 / block_round1024
of lsmblk_dev.hpp) at the sizes no other GPU test gives them: shares of more than one item in the
share form, a second round with a non-zero carry in the rounds form.

  val_scan_kernel        lookups on both sides of the workgroup's width (shares of one and of two)
  sst_open_prep_kernel   1025 SSTs: a second round whose carry lands in desc[s].blk0
  dec_scan_kernel        the two-pass decode over 64 x 1024 (+ 1) one-entry blocks: shares of one
                         tile, and thread 0's of two
  filt_scan_kernel       1024 x kFiltTile + 1 entries: the first input with a second round
  meta_scan_kernel       1024 x kMetaTile + 1 one-entry blocks: thread 0's share is two tiles

scan_units_kernel and scan_offsets_kernel have theirs in test_gpu_scan.py
(test_query_counts_and_blocks_per_unit), sst_layout_kernel in test_gpu_sst_paths.py
(test_file_layout_over_many_ssts).  tscan_top_kernel and mscan_top_kernel start a second round only
above 1024 x kTScan merge tiles / 1024 x kGScan gather tiles, which no test of a few seconds reaches:
their round loop is block_round1024, the loop that test_file_layout_over_many_ssts (one sum) and
test_filter_scan_second_round (three sums, the same totals epilogue as mscan_top_kernel) run with a
carry.

Expected values come from oracle/ only: get_cases.py's restated read, pyref.sst_open,
O.decode_blocks, pyref.compact_filter_loop, pyref.encode_block_meta.
"""
import numpy as np
import pytest
import torch

import get_cases as gc
import path_cases as pc
import scan_cases as scc
import sst_cases as sc
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch, sst
from lsm_amd._lib import LSMBLK_DEBUG_TWO_PASS_DECODE, LSMBLK_ERR_MALFORMED, lib
from oracle import oracle as O
from oracle import pyref
from test_gpu_get import corrupt, opened
from test_gpu_parity import assert_kv_equal, dev_blocks, to_dev
from test_gpu_sst_paths import meta_check

pytestmark = pytest.mark.gpu

WG = scc.kScanWg  # threads of a scan workgroup (static_assert in lsmblk_get.hip: == kWgScan)
kTile = pc.read_constants(pc._SRC, ("kTile",))["kTile"]


# ------------------------------------------------------------------------------- val_scan_kernel
@pytest.mark.parametrize("nq", [WG - 1, WG, WG + 1, 2 * WG + 1])
def test_val_scan_lookup_counts(nq):
    """nq lookups drawn from the bs256 case (FOUND, TOMBSTONE, ABSENT and filtered ones mixed): shares
    of one lookup with the last threads idle or not, and of two and three -- val_off, the gathered
    values and the statuses against the restated read."""
    c, ss = gc.case("bs256"), opened("bs256")
    exp, values, _ = gc.expected("bs256", False, False)
    sel = np.sort(np.random.default_rng(nq).permutation(len(c.keys))[:nq])
    assert len(sel) == nq
    want_vals = [values[i] for i in sel]
    found = exp["status"][sel] == gc.FOUND
    assert 0.1 * nq < found.sum() < 0.9 * nq and [v is not None for v in want_vals] == found.tolist()
    got = ss.get([c.q_sst[i] for i in sel], [c.keys[i] for i in sel], [c.read_ts[i] for i in sel])
    assert (got["status"] == exp["status"][sel]).all()
    want_off = np.concatenate([[0], np.cumsum([len(v) if v else 0 for v in want_vals])])
    assert got["val_off"].tolist() == want_off.tolist()
    assert got["values"] == want_vals


# ------------------------------------------------------------------------------- sst_open_prep_kernel
def test_open_of_1025_ssts_one_malformed():
    """WG + 1 one-block SSTs, one of the first round with its bloom offset past the file: the second
    round's SST takes its index slot from the carry, which leaves the malformed file out."""
    nsst, bad = WG + 1, 700
    ents = [(b"k%05d" % s, 5 + s % 7, b"v%d" % s) for s in range(nsst)]
    bufs = [pyref.sst_file([e], 4096) for e in ents]
    bufs[bad] = corrupt("bloom-offset-past-file", bufs[bad])
    off = [0] + np.cumsum([len(b) for b in bufs]).tolist()
    ss = sst.SstSet(b"".join(bufs), off)
    assert ss.err.tolist() == [LSMBLK_ERR_MALFORMED if s == bad else 0 for s in range(nsst)]
    assert ss.open_stats == [nsst - 1, nsst - 1, LSMBLK_ERR_MALFORMED, 0]
    good = [s for s in range(nsst) if s != bad]
    assert [int(ss.desc["blk0"][s]) for s in good] == list(range(nsst - 1))
    for s in good:
        metas, _, _, meta_offset = pyref.sst_open(bufs[s])
        assert ss.num_of_blocks(s) == 1 and ss.block_meta(s) == [(0, meta_offset, metas[0][1])]
        assert ss.first_key(s) == ents[s][0] == ss.last_key(s)
    q = [0, bad - 1, bad, bad + 1, WG - 1, WG]  # the last: the second round's SST
    got = ss.get(q, [ents[s][0] for s in q], 100, no_filter=True)
    assert got["status"].tolist() == [gc.ABSENT if s == bad else gc.FOUND for s in q]
    assert got["values"] == [None if s == bad else ents[s][2] for s in q]


# ------------------------------------------------------------------------------- dec_scan_kernel
@pytest.fixture(scope="module")
def one_entry_blocks():
    """kTile x WG + 1 one-entry blocks (block_size 16) and the oracle's decode of them."""
    n = kTile * WG + 1
    rng = np.random.default_rng(511)
    kv = sc.build([(rng.integers(4, 9, n), rng.integers(0, 4, n))], 16, 511).kv
    rc, blocks, off = O.encode_segments(kv, [0, n], 16)
    assert rc == 0 and len(off) - 1 == n
    rc, ref = O.decode_blocks(blocks, off)
    assert rc == 0 and pc.kv_equal(ref, kv)
    return blocks, off, ref


@pytest.mark.parametrize("extra", [0, 1])
def test_two_pass_decode_scan_shares(one_entry_blocks, extra):
    """LSMBLK_DEBUG_TWO_PASS_DECODE over kTile x WG blocks (every thread of dec_scan_kernel one count
    tile) and one block more (shares of two tiles, half the threads idle): stream and block entry
    index against the oracle's decode."""
    blocks, off, ref = one_entry_blocks
    nblk = kTile * WG + extra
    want = O.KV(ref.keys[:ref.key_off[nblk]], ref.key_off[:nblk + 1], ref.vals[:ref.val_off[nblk]],
                ref.val_off[:nblk + 1], ref.ts[:nblk])
    ctx = batch._ctx(0)
    assert lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_TWO_PASS_DECODE, 1) == 0
    try:
        got, ent = batch.decode_blocks(*dev_blocks(blocks[:int(off[nblk])], off[:nblk + 1]), with_blk_ent=True)
    finally:
        lib().lsmblk_debug_set(ctx, LSMBLK_DEBUG_TWO_PASS_DECODE, 0)
    assert_kv_equal(got, want)
    np.testing.assert_array_equal(ent.cpu().numpy(), np.arange(nblk + 1))


# ------------------------------------------------------------------------------- filt_scan_kernel
def test_filter_scan_second_round():
    """WG x kFiltTile + 1 entries: filt_scan_kernel's second round holds the last entry's tile alone,
    on top of the first round's carry.  Keys of 3 bytes in up to six versions, values of 0..2
    bytes, watermark inside the version range, bottom level: entries are dropped and kept in every
    tile, the last entry (a key of its own, above the watermark, one value byte) is kept, so all
    three sums are non-zero in both rounds -- against compact_generate_sst's loop."""
    n = WG * scc.kFiltTile + 1
    rng = np.random.default_rng(77)
    kid = np.repeat(np.arange(n), rng.integers(1, 7, n))[:n]
    kid[-1] = kid[-2] + 1
    rank = np.arange(n) - np.searchsorted(kid, kid)  # the version's place under its key
    ts = (1000 - 150 * rank + rng.integers(0, 150, n)).astype(np.uint64)
    vlen = np.where(rng.random(n) < 0.3, 0, rng.integers(1, 3, n))
    ts[-1], vlen[-1] = 1100, 1
    vo = np.concatenate([[0], np.cumsum(vlen)]).astype(np.uint32)
    kv = O.KV(np.ascontiguousarray(pc._be(kid, 3)).reshape(-1), (3 * np.arange(n + 1)).astype(np.uint32),
              rng.integers(0, 256, int(vo[-1]), dtype=np.uint8), vo, ts)
    kb, vb, tl, vol = kv.keys.tobytes(), kv.vals.tobytes(), ts.tolist(), vo.tolist()
    ents = [(kb[3 * i:3 * i + 3], tl[i], vb[vol[i]:vol[i + 1]]) for i in range(n)]
    kept = pyref.compact_filter_loop(ents, 700, True)
    assert 0.3 * n < len(kept) < 0.9 * n and kept[-1] == ents[-1] and len(ents[-1][2]) == 1
    got = batch.compact_filter(to_dev(kv), 700, True)
    assert_kv_equal(got, O.KV.from_entries(kept))


# ------------------------------------------------------------------------------- meta_scan_kernel
def test_block_meta_scan_shares_of_two_tiles():
    """WG x kMetaTile + 1 one-entry blocks in two segments: meta_scan_kernel's threads take two tiles
    each (the last ones none) -- the sections against pyref.encode_block_meta."""
    nb = WG * sc.C.kMetaTile + 1
    rng = np.random.default_rng(512)
    cut = nb // 2 + 3
    case = sc.build([(rng.integers(4, 7, cut), np.zeros(cut, np.int64)),
                     (rng.integers(4, 7, nb - cut), np.zeros(nb - cut, np.int64))], 16, 512)
    lay = sc.layout(case)
    assert len(lay.blk_off) - 1 == nb and lay.sst_blk.tolist() == [0, cut, nb]
    meta = torch.zeros(int(lay.meta_len.sum()) + 256, dtype=torch.uint8, device="cuda")
    meta_check(case, lay.sst_blk, lay, meta, 0, f"{nb} blocks")
