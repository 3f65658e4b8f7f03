"""The shard inputs of tests/shard_cases.py, checked on the CPU: every configuration's carry grid must reach
every branch of shard_carry_kernel it was built for (and fail that check against other constants), the oracle
must answer the whole grid and chain range after range to the single-stream compaction, the refused inputs
must be the ones the oracle has no answer for, and the bound pairs must sit on the edges their names claim.
test_gpu_shard_paths.py runs the same inputs on the device."""
import dataclasses

import numpy as np
import pytest

import compact_cases as cc
import shard_cases as sc
from oracle import oracle as O

_memo = {}


def cases():
    if "cases" not in _memo:
        _memo["cases"] = sc.ext_cases()
        _memo["answers"] = sc.all_answers(_memo["cases"])
    return _memo["cases"], _memo["answers"]


def by_config(cs):
    out = {}
    for case in cs:
        out.setdefault(case.config, []).append(case)
    return out


def test_constants_are_read_from_the_kernel_source(tmp_path):
    text = open(cc._SRC).read()
    assert sc.HALO == (16, 2) and [sc.halo_entries(bs) for bs in sc.BLOCK_SIZES] == [6, 18]
    assert sc.flevels_formula() == sc.FLEVELS_TEXT   # shard_flevels below restates exactly this loop
    assert [sc.shard_flevels(c) for c in (1, 2, 3, 4, 7, 8)] == [1, 2, 2, 3, 3, 4]
    f = tmp_path / "k.hip"
    halo, hops = "return uint64_t(block_size) / 16 + 2;", f"#define LSMBLK_ROT_HOPS {sc.C.kRotHops}\n"
    assert halo in text and hops in text
    f.write_text(text.replace(halo, "return uint64_t(block_size) / 8 + 3;")
                 .replace(hops, f"#define LSMBLK_ROT_HOPS {2 * sc.C.kRotHops}\n"))
    assert sc.halo_formula(str(f)) == (8, 3) and cc.kernel_constants(str(f)).kRotHops == 2 * sc.C.kRotHops
    f.write_text(text.replace(halo, halo.replace("+", "-")))
    with pytest.raises(RuntimeError):
        sc.halo_formula(str(f))
    f.write_text(text.replace("uint32_t shard_flevels(", "uint32_t shard_flevels_x("))
    with pytest.raises(RuntimeError):
        sc.flevels_formula(str(f))


def test_every_configuration_reaches_every_branch(tmp_path):
    cs, answers = cases()
    counts = set()
    for name, group in by_config(cs).items():
        seen, cnt = sc.check_config(group, answers)
        counts |= cnt
        print(f"{name}: block_size {group[0].bs}, target {group[0].target} ({cc.rot_levels(group[0].target, group[0].bs)} "
              f"levels), {[(c.name, c.m, c.n) for c in group]}: SSTs starting in a range {sorted(cnt)}")
    assert set(sc.SST_COUNTS) <= counts, sorted(counts)
    levels = {cc.rot_levels(t, bs) for bs, t in sc.configs().values()}
    assert 1 in levels and max(levels) >= 3
    # the constants of an edited copy of the kernel source: the three-level targets fall to two levels, a halo of
    # another length is no longer the one the cases carry -- and cases built for those constants pass again
    text = open(cc._SRC).read()
    f = tmp_path / "k.hip"
    f.write_text(text.replace(f"#define LSMBLK_ROT_HOPS {sc.C.kRotHops}\n", f"#define LSMBLK_ROT_HOPS {2 * sc.C.kRotHops}\n")
                 .replace("return uint64_t(block_size) / 16 + 2;", "return uint64_t(block_size) / 8 + 3;"))
    c2, halo2 = cc.kernel_constants(str(f)), sc.halo_formula(str(f))
    groups = by_config(cs)
    with pytest.raises(AssertionError):
        sc.check_config(groups["bs64-l3"], answers, c2)
    with pytest.raises(AssertionError):
        sc.check_config(groups["bs256-l1"], answers, halo=halo2)
    g2 = by_config(sc.ext_cases(c2, halo2))["bs64-l3"]
    sc.check_config(g2, sc.all_answers(g2), c2, halo2)


def test_the_oracle_answers_the_whole_grid_and_only_the_grid():
    """O.shard_rotation returns ORC_OK on every grid point of every stream; the inputs of the error contract are
    outside it: the oracle has no answer (ORC_E_INVAL) where the halo is short or missing without LAST, and
    answers the same ext with LAST."""
    cs, answers = cases()
    assert all(rc == O.ORC_OK for rc, _, _ in answers.values()) and len(answers) == sum(len(sc.carry_grid(c)) for c in cs)
    err = sc.error_cases()
    case, p, d0 = err["m_inside_versions"]
    assert case.m not in sc.key_changes(case.ext) and 0 < case.m < case.n
    for name in ("halo_short", "no_halo_open", "no_halo_reached"):
        case, p, d0 = err[name]
        assert case.m in sc.key_changes(case.ext) + [case.n] and p < case.m and not case.last
        assert sc.oracle_answer(case, p, d0)[0] == O.ORC_E_INVAL, name
        rc, seg, (p_out, d_out) = sc.oracle_answer(dataclasses.replace(case, last=True), p, d0)
        assert rc == O.ORC_OK and (p_out, d_out) == (case.n - case.m, 0) and seg[-1] == case.n, name
    assert err["halo_short"][0].n == err["halo_short"][0].m + 1 and err["no_halo_open"][0].n == err["no_halo_open"][0].m
    # the two no-halo inputs differ in what the open SST did: one never reaches its target, the other's chain of
    # SSTs runs through the range
    assert len(sc.oracle_answer(dataclasses.replace(err["no_halo_open"][0], last=True), 0, 0)[1]) == 2
    assert len(sc.oracle_answer(dataclasses.replace(err["no_halo_reached"][0], last=True), 0, err["no_halo_reached"][2])[1]) > 3


@pytest.mark.parametrize("config", sorted(sc.configs()))
def test_grid_answers_chain_to_the_whole_stream(config):
    """The stream of a configuration cut at key changes (a range of one key and an empty one included): each
    range's oracle answer fed forward gives O.compact's blocks and SST starts over the whole stream."""
    bs, target = sc.configs()[config]
    stream, _ = sc.version_stream(bs)
    same = sc.explicit_same(stream, 0) if config == "ex" else None
    ch = sc.key_changes(stream) if same is None else [i for i in range(1, stream.n) if not same[i]]
    pick = lambda i: sc._change_at_or_after(ch, i)
    one = pick(300)
    cuts = [0, pick(60), pick(61), one, ch[ch.index(one) + 1], ch[ch.index(one) + 1], pick(430), stream.n]
    blocks, starts = sc.chain_ranges(stream, cuts, bs, target, same)
    if same is None:
        want = O.compact(stream, np.arange(stream.n, dtype=np.uint32), 0, False, (), bs, target)
        assert blocks == want["blocks"].tobytes() and starts == want["sst_ent"][:-1].tolist()
    one_blocks, one_starts = sc.chain_ranges(stream, [0, stream.n], bs, target, same)
    assert (blocks, starts) == (one_blocks, one_starts) and len(starts) >= (3 if config.endswith("l3") else 9)


def test_sst_counts_have_a_carry_in_each():
    cs, answers = cases()
    case = next(c for c in cs if c.name == "bs64-l1-mid")
    pts = sc.sst_count_points(case, answers)
    assert set(sc.SST_COUNTS) <= set(pts), sorted(pts)
    for c in sc.SST_COUNTS[1:]:   # what the capacity contract relies on: sst_cap == c always has levels enough
        assert 2 ** sc.shard_flevels(c) >= c
    assert [cap for cap in range(1, 8) if 2 ** sc.shard_flevels(cap) < 8] == [1, 2, 3]


def test_bound_pairs_sit_on_their_edges():
    case = sc.bound_runs()
    keys = sc.check_bound_cases(case)
    print(f"bounds: {len(keys)} keys over runs of {np.diff(case.rs.astype(np.int64)).tolist()} entries, "
          f"{len(sc.bound_pairs(case))} (lo, hi) pairs")
    empty = 0
    for bottom in (False, True):   # the host predicate alone cuts every kept stream without loss or duplicate
        for mode in (sc.RUNS, sc.NEWEST, sc.TWO):
            kept = sc.kept_entries(case, mode, bottom)
            for sp in sc.splitter_sets():
                bounds = [None] + sp + [None]
                parts = [[e for e in kept if sc.in_bounds(e[0], lo, hi)] for lo, hi in zip(bounds[:-1], bounds[1:])]
                assert [e for p in parts for e in p] == kept
                empty += sum(1 for p in parts if not p)
    assert empty   # a repeated splitter: an empty range
