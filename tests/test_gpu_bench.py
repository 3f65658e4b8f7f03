"""bench.py's plain run, --full and --dump-outputs on a small batch, in process (bench.main(argv)).

A plain run prints the headline line alone; --full adds the checks and the roofline after the
timed steps; --dump-outputs writes what the last timed step returned, the same on every run, and
the dumped blocks decode (C oracle) to the dumped KV stream."""
import glob
import json
import os

import numpy as np
import pytest

import bench
from gpu_kit import _need_gpu  # noqa: F401 (autouse)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--blocks", "192", "--segment-bytes", "131072"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def run(capsys, *argv):
    capsys.readouterr()
    rc = bench.main(SMALL + list(argv))
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert rc == 0 and len(lines) == 1
    return json.loads(lines[0])


def load(d):
    return {os.path.basename(p)[:-4]: np.load(p) for p in sorted(glob.glob(os.path.join(d, "*.npy")))}


def test_plain_run_prints_the_headline_alone(capsys):
    line = run(capsys, "--steps", "3", "--warmup", "1")
    assert all(k in line for k in HEADLINE)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False and line["status_ok"] is True
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    E = line["config"]["encoded_bytes_per_gpu"]
    assert line["value"] == pytest.approx(E / (line["ms_per_step"] * 1e-3) / 2 ** 30, rel=5e-3)
    for k in ("roofline", "cpu_baseline", "pcie_inclusive", "extra_configs", "framing_crc32"):
        assert k not in line
    assert "oracle_checked_blocks" not in line["config"]


def test_full_run_checks_and_profiles(capsys):
    line = run(capsys, "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-pcie")
    assert all(k in line for k in HEADLINE) and line["full"] is True and line["steps"] == 2
    assert line["config"]["roundtrip_bit_exact"] is True and line["config"]["oracle_checked_blocks"] == 192
    assert line["roofline"]["kernel"] in line["roofline"]["kernels_ms"] and line["roofline"]["launch_ms"] > 0
    assert line["framing_crc32"]["ok"] and line["encode_framed"]["verified"]


def test_dump_outputs_is_the_last_step_and_repeats(capsys, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    la = run(capsys, "--steps", "2", "--warmup", "1", "--dump-outputs", a)
    run(capsys, "--steps", "1", "--warmup", "0", "--dump-outputs", b)
    da, db = load(a), load(b)
    assert set(da) == {"keys", "key_off", "vals", "val_off", "ts", "decode_stats", "blocks", "blk_off", "encode_stats"}
    assert set(db) == set(da) and all(np.array_equal(da[k], db[k]) for k in da)
    assert all(v.dtype == (np.float32 if k in ("keys", "vals", "blocks") else np.float64) for k, v in da.items())
    n, nblk, E = (la["config"][k] for k in ("entries_per_gpu", "blocks_per_gpu", "encoded_bytes_per_gpu"))
    assert len(da["ts"]) == n and len(da["blk_off"]) == nblk + 1 and len(da["blocks"]) == E  # small: whole arrays
    assert da["decode_stats"][0] == n and da["decode_stats"][3] == 0
    assert da["encode_stats"][0] == nblk and da["encode_stats"][1] == E and da["encode_stats"][3] == 0
    # the dumped blocks, decoded by the oracle, are the dumped KV stream
    rc, kv = O.decode_blocks(da["blocks"].astype(np.uint8), da["blk_off"].astype(np.uint64))
    assert rc == 0 and kv.n == n
    assert np.array_equal(kv.keys, da["keys"].astype(np.uint8)) and np.array_equal(kv.vals, da["vals"].astype(np.uint8))
    assert np.array_equal(kv.key_off, da["key_off"].astype(np.uint32))
    assert np.array_equal(kv.val_off, da["val_off"].astype(np.uint32))
    assert np.array_equal(kv.ts, da["ts"].astype(np.uint64))


def test_dump_outputs_samples_large_arrays_within_the_budget(capsys, tmp_path, monkeypatch):
    """Arrays longer than the element budget are written as the same sorted sample on every run."""
    assert bench.DUMP_BYTES <= 60 << 20
    whole = str(tmp_path / "w")
    run(capsys, "--steps", "1", "--warmup", "0", "--dump-outputs", whole)
    monkeypatch.setattr(bench, "DUMP_BYTES", 60 * 1000)  # 60 B of items per index: 1000 elements per array
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    run(capsys, "--steps", "1", "--warmup", "0", "--dump-outputs", a)
    run(capsys, "--steps", "1", "--warmup", "0", "--dump-outputs", b)
    dw, da, db = load(whole), load(a), load(b)
    assert all(np.array_equal(da[k], db[k]) for k in da)
    assert sum(v.nbytes for v in da.values()) <= 60 * 1000
    for k in ("keys", "vals", "blocks", "key_off", "val_off", "ts"):
        assert len(da[k]) == 1000 < len(dw[k])
    for k in ("key_off", "val_off"):  # a sample at sorted indices of a rising table rises
        assert np.all(np.diff(da[k]) >= 0) and da[k][0] >= dw[k][0] and da[k][-1] <= dw[k][-1]
    assert np.isin(da["ts"], dw["ts"]).all()
    assert all(np.array_equal(da[k], dw[k]) for k in ("blk_off", "decode_stats", "encode_stats"))
