"""Static check on the gfx950 ISA of the decode's large-block value copy (CPU only: hipcc
cross-compiles).

copy_long_runs<kDecBigB> keeps kDecBigB 16-B loads per lane in flight before their stores (config
M's decode is this loop).  The loads must be issued back to back: an `s_waitcnt vmcnt` between two of
them makes each wait for the one before, one load in flight instead of kDecBigB.  That happened when
the register allocator used a load's destination registers, which are also the data of the previous
round's stores, as scratch for the load's address ("Decode: values compacted in
place"); copy_issue<B, true> now claims the registers first and issues the loads by inline asm.

A copy batch is recognised as a group of `buffer_load_dwordx4 ..., 0 offen` without an immediate
offset from one descriptor, each within 40 lines of the one before (a piece's owner lookup and address
arithmetic lie between two loads); the staging loads carry immediate offsets and do not form one."""
import os
import re
import subprocess

import pytest

import decode_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LOAD = re.compile(r"buffer_load_dwordx4 v\[(\d+):\d+\], v(\d+), (s\[\d+:\d+\]), 0 offen$")
WAIT = re.compile(r"s_waitcnt\b.*\bvmcnt")


def kernel_body(lines, name):
    st = [i for i, ln in enumerate(lines) if re.match(r"^_ZN\S*\d+%sE\S*:" % name, ln)]
    assert len(st) == 1, (name, st)
    end = next(i for i in range(st[0], len(lines)) if "s_endpgm" in lines[i])
    return [ln.strip() for ln in lines[st[0] + 1:end]]


def copy_groups(body):
    """[(loads, vmcnt waits between the first and the last, loads addressed from their own destination)]"""
    loads = [(i, LOAD.match(t)) for i, t in enumerate(body)]
    loads = [(i, m) for i, m in loads if m]
    groups, cur = [], []
    for i, m in loads:
        if cur and (m.group(3) != cur[-1][1].group(3) or i - cur[-1][0] > 40):
            groups.append(cur)
            cur = []
        cur.append((i, m))
    if cur:
        groups.append(cur)
    out = []
    for g in groups:
        if len(g) >= 4:
            waits = sum(1 for k in range(g[0][0], g[-1][0]) if WAIT.match(body[k]))
            out.append((len(g), waits, sum(m.group(1) == m.group(2) for _, m in g)))
    return out


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("isa")
    out = d / "lsmblk_gpu.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/include", "-DLSMBLK_DIAG_BUILD=0",
                    "--offload-device-only", "-S", "-o", str(out), os.path.join(ROOT, "lsm_amd", "csrc", "lsmblk_gpu.hip")],
                   check=True, capture_output=True, cwd=str(d))
    return out.read_text().split("\n")


@pytest.mark.parametrize("kernel", ("decode_kernel", "decode_lag_kernel"))
def test_copy_batch_loads_are_issued_back_to_back(isa, kernel):
    groups = copy_groups(kernel_body(isa, kernel))
    # dec_big_outputs is inlined at its two call sites: two batches of kDecBigB loads
    assert [n for n, _, _ in groups] == [dc.C.kDecBigB] * 2, groups
    assert all(w == 0 and own == 0 for _, w, own in groups), groups


def test_the_check_sees_a_serialised_batch():
    """The recogniser on a hand-written fragment of the faulty shape: the address in the load's own
    destination and a wait in front of every load."""
    body = []
    for j in range(8):
        r = 2 + 4 * j
        body += ["s_waitcnt vmcnt(0)", f"v_lshlrev_b32_e32 v{r}, 4, v56", f"ds_read_b128 v[80:83], v{r} offset:4128",
                 "s_waitcnt lgkmcnt(0)", f"v_add_u32_e32 v{r}, v54, v80",
                 f"buffer_load_dwordx4 v[{r}:{r + 3}], v{r}, s[28:31], 0 offen"]
    assert copy_groups(body) == [(8, 7, 8)]
