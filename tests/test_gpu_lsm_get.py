"""Point reads over an LSM view on the device (lsmblk_lsm_get_batch; lsm_amd.sst.SstSet.lsm_get) against
the CPU expectations of lsm_get_cases.py: every field of every result in the three modes, the
stats, the gathered values and the capacity contract, the view check's reports, and the composition
it replaces (SstSet.get per (table, key), folded on the host)."""
import bisect
import ctypes

import numpy as np
import pytest
import torch

import gpu_kit as kit
import lsm_get_cases as lc
import scan_cases as sc
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from lsm_amd import batch, sst
from lsm_amd._lib import (LSMBLK_ERR_CAPACITY, LSMBLK_ERR_EMPTY_KEY, LSMBLK_ERR_MALFORMED, LSMBLK_ERR_SEGMENTS,
                          LSMBLK_E_INVAL, LSMBLK_GET_NO_FILTER, LsmBlkError, LsmGetResultC)
from oracle import pyref
from test_gpu_get import capacity_retry_case, check_capacity_retry

pytestmark = pytest.mark.gpu


def opened(name, bs):
    """(the case, its SstSet, its view); one mixed / edges set per block size."""
    v = lc.case(name, bs)
    return (v, *kit.opened_view(v, ("lsm_get", name, bs)))


def check_fields(got, exp, keys, what=""):
    for f in lc.FIELDS:
        bad = np.nonzero(got[f].astype(np.uint64) != exp[f])[0]
        assert not len(bad), (what, f, bad[:5], [keys[i] for i in bad[:5]], got[f][bad[:5]], exp[f][bad[:5]])


def check_refused(r, vo, st, nq, flag):
    """The view check's verdict: no lookup ran."""
    assert st == [nq, 0, 0, flag]
    assert (r["status"] == lc.ABSENT).all() and (r["vlen"] == 0).all() and (r["seeks"] == 0).all()
    assert (r["bloom_out"] == 0).all()
    for f in ("src", "sst", "hit_blk", "hit_ent"):
        assert (r[f] == lc.NONE).all(), f
    assert vo.tolist() == [0] * (nq + 1)


@pytest.mark.parametrize("mode", lc.MODES)
@pytest.mark.parametrize("name,bs", lc.CASES)
def test_every_field_equals_the_expectation(name, bs, mode):
    v, ss, view = opened(name, bs)
    exp, values, val_off = lc.expected(name, bs, mode)
    need, nq = int(val_off[-1]), len(v.keys)
    vals = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    r, _, vo, st = ss.lsm_get_raw(view, v.keys, v.read_ts, lc.FLAGS[mode], val_cap=need, vals=vals)  # exact capacity
    check_fields(r, exp, v.keys)
    assert st == [nq, int((exp["status"] == lc.FOUND).sum()), need, 0]
    assert vo.tolist() == val_off.tolist()
    assert vals[:need].cpu().numpy().tobytes() == b"".join(x for x in values if x) and (vals[need:] == 0xAB).all()
    files = v.files
    for i in np.nonzero(r["status"] == lc.FOUND)[0][:200]:  # val_pos / vlen point at the same bytes
        assert files[int(r["val_pos"][i]):int(r["val_pos"][i]) + int(r["vlen"][i])] == values[i]
    out = ss.lsm_get(view, v.keys, v.read_ts, mvcc=mode == "mvcc", newest=mode == "newest")
    assert out["values"] == values and all((out[f] == r[f]).all() for f in lc.FIELDS)


@pytest.mark.parametrize("mode", lc.MODES)
def test_capacity_contract_and_repeatability(mode):
    v, ss, view = opened("mixed", 128)
    exp, values, val_off = lc.expected("mixed", 128, mode)
    need, nq = int(val_off[-1]), len(v.keys)
    assert need > 1
    vals = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    r, _, vo, st = ss.lsm_get_raw(view, v.keys, v.read_ts, lc.FLAGS[mode], val_cap=need - 1, vals=vals)  # one byte short
    assert st[3] == LSMBLK_ERR_CAPACITY and st[2] == need and st[0] == nq and (vals == 0xAB).all()
    check_fields(r, exp, v.keys, "short")
    r2, none, vo2, st2 = ss.lsm_get_raw(view, v.keys, v.read_ts, lc.FLAGS[mode])  # vals = NULL
    assert none is None and vo2 is None and st2[3] == 0 and st2[0] == nq and st2[1] == int((exp["status"] == lc.FOUND).sum())
    check_fields(r2, exp, v.keys, "no gather")
    r3, _, _, st3 = ss.lsm_get_raw(view, v.keys, v.read_ts, lc.FLAGS[mode])  # the same context again
    assert r3.tobytes() == r2.tobytes() and st3 == st2


def test_empty_batch():
    _, ss, view = opened("mixed", 128)
    r, _, vo, st = ss.lsm_get_raw(view, [], [], val_cap=16)
    assert st == [0, 0, 0, 0] and len(r) == 0 and vo.tolist() == [0]
    out = ss.lsm_get(view, [], [])
    assert out["values"] == [] and len(out["status"]) == 0


def test_an_empty_key_is_reported_and_the_others_answer():
    v, ss, view = opened("mixed", 128)
    exp, _, _ = lc.expected("mixed", 128, "default")
    keys = list(v.keys[:40])
    keys[7] = b""
    r, _, _, st = ss.lsm_get_raw(view, keys, v.read_ts[:40])
    assert st[3] == LSMBLK_ERR_EMPTY_KEY and st[0] == 40
    assert r["status"][7] == lc.ABSENT and r["src"][7] == lc.NONE and r["seeks"][7] == 0
    ok = np.arange(40) != 7
    for f in lc.FIELDS:
        assert (r[f][ok].astype(np.uint64) == exp[f][:40][ok]).all(), f


def test_no_filter_is_refused():
    v, ss, view = opened("mixed", 128)
    with pytest.raises(LsmBlkError) as e:
        ss.lsm_get_raw(view, v.keys[:4], v.read_ts[:4], LSMBLK_GET_NO_FILTER)
    assert e.value.status == LSMBLK_E_INVAL


def into(ss, view, keys, read_ts, flags, lead):
    """lsm_get_into with the key arena starting `lead` bytes past a 16-byte boundary."""
    nq = len(keys)
    kb = b"".join(keys)
    arena = batch._aligned_empty(len(kb) + 32, ss.device)
    qk = arena[lead:lead + len(kb) + 1]
    qk[:len(kb)].copy_(torch.frombuffer(bytearray(kb), dtype=torch.uint8))
    assert qk.data_ptr() % 4 == lead % 4
    qo = batch._u32_table(np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint32), ss.device)
    qt = torch.from_numpy(np.asarray(read_ts, np.uint64).view(np.int64)).to(ss.device)
    res = torch.zeros(nq * ctypes.sizeof(LsmGetResultC), dtype=torch.uint8, device=ss.device)
    stats = torch.zeros(batch.STATS_WORDS, dtype=torch.int64, device=ss.device)
    ss.lsm_get_into(view, qk, qo, qt, nq, flags, res, stats)
    torch.cuda.synchronize()
    return res.cpu().numpy().view(np.dtype(LsmGetResultC)), stats.cpu().tolist()


@pytest.mark.parametrize("lead", (0, 1, 2, 3))
def test_key_arena_at_every_address_residue(lead):
    v, ss, view = opened("edges_l0", 256)
    exp, _, _ = lc.expected("edges_l0", 256, "mvcc")
    r, st = into(ss, view, v.keys, v.read_ts, lc.FLAGS["mvcc"], lead)
    assert st[3] == 0
    check_fields(r, exp, v.keys, lead)


def test_every_wave_answers_several_keys():
    """More than 2 x 32 x CUs lookups, so every wave's grid-stride loop runs at least twice; a found
    key is followed by an absent one and a bloom-rejected one, so stale per-key state would show."""
    v, ss, view = opened("mixed", 128)
    rws = lc.rows("mixed", 128, "default")
    found = [i for i, r in enumerate(rws) if r["status"] == lc.FOUND]
    absent = [i for i, r in enumerate(rws) if r["status"] == lc.ABSENT and r["bloom_out"] == 0]  # no filter rejected it
    rejected = [i for i, r in enumerate(rws) if r["src"] == lc.NONE and r["seeks"] == 0 and r["bloom_out"] > 0]
    assert min(len(found), len(absent), len(rejected)) >= 20
    order = [i for t in zip(found, absent, rejected) for i in t]
    order += sorted(set(range(len(rws))) - set(order))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    order = order * (2 * 32 * cus // len(order) + 1)
    assert len(order) > 2 * 32 * cus
    keys, ts = [v.keys[i] for i in order], [v.read_ts[i] for i in order]
    for mode in lc.MODES:
        exp, _, _ = lc.arrays(v, [lc.rows("mixed", 128, mode)[i] for i in order])
        r, _, _, st = ss.lsm_get_raw(view, keys, ts, lc.FLAGS[mode])
        assert st[3] == 0 and st[0] == len(order)
        check_fields(r, exp, keys, mode)


@pytest.mark.parametrize("mode", lc.MODES)
def test_agrees_with_per_table_gets_folded_on_the_host(mode):
    """The composition the call replaces: the (table, key) expansion with every level bisected on the
    host, one SstSet.get over it, the fold."""
    v, ss, view = opened("mixed", 256)
    firsts = [[ss.first_key(t) for t in lv] for lv in v.levels]
    q_sst, qk, qt, owner = [], [], [], []
    for i, (key, ts) in enumerate(zip(v.keys, v.read_ts)):
        for src in range(v.nsrc):
            if src < len(v.l0):
                t = v.l0[src]
            else:
                p = bisect.bisect_right(firsts[src - len(v.l0)], key)
                if p == 0:
                    continue
                t = v.levels[src - len(v.l0)][p - 1]
            q_sst.append(t)
            qk.append(key)
            qt.append(ts)
            owner.append((i, src))
    g = ss.get(q_sst, qk, qt, mvcc=mode != "default", values=False)
    fold = [dict(status=lc.ABSENT, src=lc.NONE, sst=lc.NONE, hit_blk=lc.NONE, hit_ent=lc.NONE, vlen=0, ts=0, val_pos=0,
                 seeks=0, bloom_out=0, done=False) for _ in v.keys]
    for j, (i, src) in enumerate(owner):
        f, status = fold[i], int(g["status"][j])
        if f["done"] or status == lc.RANGE_OUT:
            continue
        if status == lc.BLOOM_OUT:
            f["bloom_out"] += 1
            continue
        f["seeks"] += 1
        hit = dict(status=status, src=src, sst=q_sst[j], **{x: int(g[x][j]) for x in ("hit_blk", "hit_ent", "vlen", "ts", "val_pos")})
        if mode != "newest":
            blocks, b, e = v.ssts[q_sst[j]].blocks, int(g["blk"][j]), int(g["ent"][j])
            if b < len(blocks) and blocks[b][e][0] == qk[j]:
                f.update(hit, done=True)
        elif status != lc.ABSENT and (f["src"] == lc.NONE or hit["ts"] > f["ts"]):
            f.update(hit)
    got = ss.lsm_get(view, v.keys, v.read_ts, mvcc=mode == "mvcc", newest=mode == "newest", values=False)
    for f in lc.FIELDS:
        want = np.array([x[f] for x in fold], np.uint64)
        bad = np.nonzero(got[f].astype(np.uint64) != want)[0]
        assert not len(bad), (f, bad[:5], got[f][bad[:5]], want[bad[:5]])


# ------------------------------------------------------------------------------ the view check
def refused(ss, view, v, flag):
    nq = 64
    for flags in (0, lc.FLAGS["newest"]):
        r, _, vo, st = ss.lsm_get_raw(view, v.keys[:nq], v.read_ts[:nq], flags, val_cap=4096)
        check_refused(r, vo, st, nq, flag)
    with pytest.raises(LsmBlkError):
        ss.lsm_get(view, v.keys[:nq], v.read_ts[:nq])


def test_view_with_an_id_past_the_set():
    v, ss, _ = opened("mixed", 128)
    refused(ss, ss.view(v.l0 + [ss.nsst], v.levels), v, LSMBLK_ERR_SEGMENTS)
    refused(ss, ss.view(v.l0, [v.levels[0], v.levels[1][:-1] + [0xFFFFFFF0]]), v, LSMBLK_ERR_SEGMENTS)


def test_view_with_a_decreasing_level_start():
    v, ss, _ = opened("mixed", 128)
    view = ss.view(v.l0, v.levels)
    view.level_start_t = batch._u32_table(np.array([0, 5, 3], np.uint32), ss.device)
    refused(ss, view, v, LSMBLK_ERR_SEGMENTS)
    view.level_start_t = batch._u32_table(np.array([1, 3, 7], np.uint32), ss.device)  # [0] != 0
    refused(ss, view, v, LSMBLK_ERR_SEGMENTS)


def test_view_with_swapped_neighbours():
    v, ss, _ = opened("mixed", 128)
    a = v.levels[1]
    refused(ss, ss.view(v.l0, [v.levels[0], [a[0], a[2], a[1], a[3]]]), v, LSMBLK_ERR_MALFORMED)


def test_view_with_overlapping_neighbours():
    v, ss, _ = opened("mixed", 128)
    x, y = sorted(v.l0[:2], key=lambda t: lc.first_key(v.ssts[t]))
    assert lc.first_key(v.ssts[x]) < lc.first_key(v.ssts[y]) <= lc.last_key(v.ssts[x])
    refused(ss, ss.view([v.l0[2]], [v.levels[0], [x, y]]), v, LSMBLK_ERR_MALFORMED)
    # the same two tables in different levels are a valid view
    r, _, _, st = ss.lsm_get_raw(ss.view([v.l0[2]], [[x], [y]]), v.keys[:64], v.read_ts[:64])
    assert st[3] == 0 and st[0] == 64


@pytest.mark.parametrize("where", ("l0", "level"))
def test_view_with_a_table_whose_open_failed(where):
    v = lc.case("mixed", 128)
    bad = v.l0[1] if where == "l0" else v.levels[1][2]
    ss = sst.SstSet(b"".join(sc.corrupt_footer(s.buf) if t == bad else s.buf for t, s in enumerate(v.ssts)), v.file_off)
    assert ss.err[bad] == LSMBLK_ERR_MALFORMED and ss.open_stats[0] == len(v.ssts) - 1
    refused(ss, ss.view(v.l0, v.levels), v, LSMBLK_ERR_MALFORMED)
    # a view of the same set without that table answers
    l0 = [t for t in v.l0 if t != bad]
    levels = [[t for t in lv if t != bad] for lv in v.levels]
    r, _, _, st = ss.lsm_get_raw(ss.view(l0, levels), v.keys, v.read_ts)
    rws = [lc.closed(lc.View("", v.ssts, l0, levels, [], []), k, ts, "default") for k, ts in zip(v.keys, v.read_ts)]
    assert st[3] == 0
    check_fields(r, lc.arrays(v, rws)[0], v.keys)


def test_lsm_get_retries_once_on_capacity():
    """Found values of 6144 bytes against the wrapper's first buffer of 64 * 4 + 1024."""
    ents, keys = capacity_retry_case()
    buf = pyref.sst_file(ents, 4096)
    ss = sst.SstSet(buf, [0, len(buf)])
    view = ss.view([0], [])
    statuses = [lc.FOUND, lc.FOUND, lc.ABSENT, lc.FOUND]
    check_capacity_retry(ss, "lsm_get_raw", lambda: ss.lsm_get(view, keys, 100), ents, keys, statuses)
