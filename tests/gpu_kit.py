"""What the GPU tests of the read path share -- TEST INFRASTRUCTURE (a plain module, not a conftest).

  _need_gpu        the module-scoped autouse fixture; a test module applies it by importing it
  guarded ...      KV streams of sentinels and the checks that nothing wrote them
  check_stream ... a stream / a result array against rows in the form of scan_cases.stream_of
  opened_view      one SstSet (and LsmView) per case, opened once per process
"""
import numpy as np
import pytest
import torch

import scan_cases as sc
from lsm_amd import batch, sst

GUARD = 0xAB


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def guarded(n, kb, vb, dev="cuda", lead=0):
    """A stream whose every word is a sentinel, its arenas `lead` bytes past a 16-byte boundary."""
    return batch.KVStream(torch.full((kb + 64 + lead,), GUARD, dtype=torch.uint8, device=dev)[lead:],
                          torch.full((n + 2,), -1, dtype=torch.int32, device=dev),
                          torch.full((vb + 64 + lead,), GUARD, dtype=torch.uint8, device=dev)[lead:],
                          torch.full((n + 2,), -1, dtype=torch.int32, device=dev),
                          torch.full((n + 1,), -1, dtype=torch.int64, device=dev), 0)


def untouched(kv, offsets=True):
    ok = bool((kv.keys == GUARD).all() and (kv.vals == GUARD).all() and (kv.ts == -1).all())
    return ok and (not offsets or bool((kv.key_off == -1).all() and (kv.val_off == -1).all()))


def all_empty(r, seg, nq):
    assert (r["status"] == sc.EMPTY).all() and seg.tolist() == [0] * (nq + 1)
    for f in ("sources", "raw", "merged", "n"):
        assert (r[f] == 0).all(), f


def sizes_of(rows):
    kb, ko, vb, vo, ts, seg = sc.stream_of(rows)
    return len(ts), len(kb), len(vb)


def check_results(r, exp, fields, sel=None):
    for f in fields:
        want = exp[f] if sel is None else exp[f][sel]
        bad = np.nonzero(r[f].astype(np.uint64) != want)[0]
        assert not len(bad), (f, bad[:5], r[f][bad[:5]], want[bad[:5]])


def check_stream(kv, rows, seg=None):
    kb, ko, vb, vo, ts, want_seg = sc.stream_of(rows)
    if seg is not None:
        assert seg.tolist() == want_seg.tolist()
    assert kv.n == len(ts)
    gk, gko, gv, gvo, gts = kv.to_numpy()
    assert gko.tolist() == ko.tolist() and gvo.tolist() == vo.tolist() and gts.tolist() == ts.tolist()
    assert gk.tobytes() == kb and gv.tobytes() == vb


_sets = {}


def opened_set(case_view, key):
    """The SstSet of case_view's files (.files, .file_off, .ssts), opened once per key."""
    if key not in _sets:
        ss = sst.SstSet(case_view.files, case_view.file_off)
        assert ss.open_stats[0] == len(case_view.ssts) and ss.open_stats[3] == 0
        _sets[key] = ss
    return _sets[key]


def opened_view(case_view, key, mem=None, set_key=None):
    """(the SstSet of case_view's tables, its LsmView over .l0 and .levels), opened once per key.  mem: a
    callable giving the view's memtable runs on a miss; set_key: the key of the set (default: key), for
    views that differ in their runs alone and share one set."""
    ss = opened_set(case_view, ("tables",) + (key if set_key is None else set_key))
    if key not in _sets:
        _sets[key] = ss.view(case_view.l0, case_view.levels, mem() if mem is not None else None)
    return ss, _sets[key]
