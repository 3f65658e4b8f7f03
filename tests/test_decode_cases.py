"""The decode-route inputs of tests/decode_cases.py, checked on the CPU: every generator's batch is
read by the C oracle and by pyref.block_entries, which must agree block for block; the model's
events under nominal addresses (an aligned base plus each lead) must hold everything the generator
was built for; a retuned constant or a cut-down generator must fail that; and the model's block
path is held against path_cases.classify.  test_gpu_decode_routes.py runs the same batches on the
device.  The guards of the decode that no valid block reaches are stated here as assertions."""
import re

import numpy as np
import pytest

import decode_cases as dc
import path_cases as pc
from oracle import oracle as O

NAMES = tuple(dc.GENERATORS)


@pytest.fixture(scope="module")
def batches():
    return {name: gen() for name, gen in dc.GENERATORS.items()}


def retuned(tmp_path, pattern, repl):
    """A copy of the kernel source with one line changed -> its constants."""
    with open(dc.GPU_SRC) as f:
        text, k = re.subn(pattern, repl, f.read(), flags=re.M)
    assert k == 1, pattern
    f = tmp_path / "retuned.hip"
    f.write_text(text)
    return dc.kernel_constants(str(f))


def test_constants_are_read_from_the_kernel_source(tmp_path):
    c = dc.C
    assert (c.kDecImg, c.kDecMaxE, c.kDecOut, c.kTile) == (pc.kDecImg, pc.kDecMaxE, pc.kDecOut, pc.kTile)
    assert c.kLB > 0 and c.kBigB > 0 and c.kDecBigB > 0 and c.kCoop > 0
    assert c.kCopyScratch == 4 * 64 + 64 and 4 * c.kCopyScratch <= c.kDecOut
    assert retuned(tmp_path, r"^#define LSMBLK_XDBB \d+$", "#define LSMBLK_XDBB 4").kDecBigB == 4
    f = tmp_path / "k.hip"
    f.write_text("constexpr uint32_t kDecImg = 1;\n")
    with pytest.raises(RuntimeError):
        dc.kernel_constants(str(f))


@pytest.mark.parametrize("name", NAMES)
def test_generator_is_valid_and_covers_its_routes(batches, name):
    """The oracle takes every block (rc 0) and reads what pyref.block_entries reads; the coverage
    of the generator holds; the model's block paths are path_cases.classify's."""
    b = batches[name]
    rc, kv = O.decode_blocks(b.blocks, b.blk_off)
    assert rc == 0
    want = b.entries()
    assert kv.n == len(want) and kv.entries() == [(bytes(k), t, bytes(v)) for k, t, v in want]
    assert int(kv.key_off[-1]) == b.K and int(kv.val_off[-1]) == b.V
    np.testing.assert_array_equal(kv.key_off[np.cumsum([0] + [dc.parse(x)[0] for x in b.bufs])[:-1]], b.K0)
    miss, ev = dc.check(name, b)
    print(dc.coverage_line(name, b, ev))
    assert not miss, miss[:20]
    for ld in dc.GEN_LEADS[name]:
        paths = dc.model_batch(b, 256 + ld)[1]
        p = pc.classify(b.blocks, b.blk_off, kv.key_off, kv.val_off, blk_addr=256 + ld)
        assert paths == [pc.DEC_PATHS[i] for i in p.dec], ld


def test_every_generator_path(batches):
    """All five block paths are reached between the generators."""
    seen = set()
    for name, b in batches.items():
        seen |= set(dc.model_batch(b)[1])
    assert seen == set(pc.DEC_PATHS)


@pytest.mark.parametrize("what", ["kDecBigB", "kLB", "kDecMaxE"])
def test_retuned_constant_fails_the_coverage(batches, tmp_path, what):
    """The batches are built for today's constants: against a retuned kernel source their coverage
    has holes, so a retune cannot silently leave the edges."""
    if what == "kDecBigB":
        c, name = retuned(tmp_path, r"^#define LSMBLK_XDBB \d+$", "#define LSMBLK_XDBB 4"), "large"
        hole = ("clr-total", 64 * 4)
    elif what == "kLB":
        c, name = retuned(tmp_path, r"^constexpr uint32_t kLB = \d+;", "constexpr uint32_t kLB = 4;"), "values"
        hole = ("flush-whole", "=")
    else:
        c, name = retuned(tmp_path, r"^constexpr uint32_t kDecMaxE = \d+;", "constexpr uint32_t kDecMaxE = 64;"), "values"
        hole = ("second-half", "lds", 64)
    assert getattr(c, what) != getattr(dc.C, what)
    miss, _ = dc.check(name, batches[name], c=c)
    assert hole in miss, miss[:20]
    assert not dc.check(name, batches[name])[0]


def test_cut_down_generator_fails_the_coverage():
    """Values and keys stepping by 4, as a U stream's 100-byte values make them: every cut is 4, 8,
    12 or 16, a quarter of the (vD & 15, vl & 15) pairs at most -- what the suite had before."""
    b = dc.values_fast(step4=True)
    rc, _ = O.decode_blocks(b.blocks, b.blk_off)
    assert rc == 0
    ev = dc.model_leads(b, dc.LEADS, only="valn")
    miss = dc.check_values(ev)
    cuts = {e[1] for e in ev if e[0] == "cut"}
    assert cuts <= {4, 8, 12, 16}, cuts
    assert ("cut", 1, "next") in miss and ("cut", 15, "last") in miss and ("vpair", 1, 1) in miss
    assert len([e for e in ev if e[0] == "vpair"]) <= 16


def test_guards_that_no_valid_block_reaches(batches):
    """Three guards stay in the kernels without an input ("Decode validity rules" bound
    what a valid block can hold):

    valn's `l == 0 && vS < (vD & 15)`: vS = lead + epos + 14 + s.  The entry at data position 0 has
    p <= fks = its own s and p + s > 0, so s >= 1 and vS >= 15; any other entry starts behind it,
    epos >= 14 + s0 >= 15.  vD & 15 <= 15.  The same bound keeps the neighbour read's source a1 =
    vS1 - cut >= 15 - 15 (reached with equality by impossible()'s fast-a1 blocks at lead 0).

    copy_run's loop for len >= 16: both callers pass only len < 16 (copy_run1 for len < 16,
    dec_big_outputs for vl < kCoop, and kCoop <= 16).

    dec_simple_outputs on the descriptor image: decode_block takes it when the block is neither
    fast, nor big, nor fits -- and big is !fits."""
    least = min(lead + epos + 14 + s for lead in range(16) for epos, s in [(0, s) for s in range(1, 4)] +
                [(14 + s0, s) for s0 in range(1, 4) for s in range(0, 3)])
    assert least == 15 >= max(vd & 15 for vd in range(64))
    assert dc.C.kCoop <= 16
    for name, b in batches.items():
        ev = dc.model_leads(b, range(16))
        assert not [e for e in ev if e[0] == "copy_run-long"], name
        assert ("valn-term", "lane0") not in ev, name
        assert not [e for e in ev if e[0] == "a1" and e[1] < 0], name
    chain = {(fits, small): ("fast" if fits and small else "tables" if not fits and small else "chunked" if not fits
                             else "simple-lds" if fits else "simple-global")
             for fits in (False, True) for small in (False, True)}
    assert "simple-global" not in chain.values()
