"""The key order of lsm_amd/csrc/lsmblk_keys.hpp, exhaustively on a CPU (no GPU: hipcc builds the
host half of tests/key_order_host.hip with the address and undefined-behaviour sanitizers).

The program instantiates every template of the keys section over the host accessor and holds it to a
plain byte loop for all ordered pairs of a key family that puts a real 0x00 against the image's pad,
a difference at bytes 15, 16 and 17, prefix pairs and every length class on both sides of each
compare, at arena leads 0..15 and once with the second key ending the arena."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_key_order_on_the_host(tmp_path):
    exe = tmp_path / "key_order_host"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-DLSMBLK_DIAG_BUILD=0",
                    f"-I{ROOT}/include", f"-I{ROOT}/lsm_amd/csrc", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "key_order_host.hip"),
                    "-o", str(exe)], check=True, capture_output=True, cwd=str(tmp_path))
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("key_order_host:")]
    assert len(line) == 1, r.stdout
    n = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", line[0])}
    # every ordered pair, none skipped, at 16 leads and the exact placement
    assert n["pairs"] == n["keys"] ** 2 and n["placements"] == 17 * n["pairs"] and n["skipped"] == 0
    # the classes a slip hides in: image ties decided by the lengths and by the tails (whose callable
    # must have run), the one-load builder and its fallback at the arena's end, reads past the bound
    for k in ("len_ties", "tail_ties", "tail_calls", "load16", "fallback", "past_bound"):
        assert n[k] > 0, (k, line[0])
