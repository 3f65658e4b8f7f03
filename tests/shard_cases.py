"""Inputs that put the key-range shard calls of lsmblk_compact.hip on chosen branches -- TEST INFRASTRUCTURE.

The method of compact_cases.py for lsmblk_compact_merge_batch[_ex] with a range, lsmblk_shard_rotation_prepare[_ex],
lsmblk_shard_rotation_carry and lsmblk_shard_encode_batch; shared by test_shard_cases.py (CPU) and
test_gpu_shard_paths.py (GPU):

  constants    compact_cases.C (kRotHops decides rot_levels), the halo formula and shard_flevels read out of the
               kernel source
  generators   extended streams (a range's own m entries, then its halo), the carry grid over them, the inputs
               that must be refused, and run sets with (lo, hi) bounds on every edge of lo <= key < hi
  classifiers  classify() names the branch of shard_carry_kernel a grid point lands on from the oracle's answer
               and position arithmetic on ext.  They only ASSERT COVERAGE; expected output comes from oracle/
               alone (O.shard_rotation, O.encode_span, O.merge_runs, O.compact, pyref's two-level iterator).
"""
import re
from dataclasses import dataclass

import numpy as np

import compact_cases as cc
import merge_newest_cases as mn
from lsm_amd._lib import (LSMBLK_MERGE_NEWEST, LSMBLK_MERGE_RUNS, LSMBLK_MERGE_TWO_LEVEL, LSMBLK_TWO_END_ABOVE,
                          LSMBLK_TWO_END_BELOW, LSMBLK_TWO_END_IN_RANGE)
from oracle import oracle as O
from oracle import pyref

C = cc.C
RUNS, TWO, NEWEST = LSMBLK_MERGE_RUNS, LSMBLK_MERGE_TWO_LEVEL, LSMBLK_MERGE_NEWEST
BLOCK_SIZES = (64, 256)
SST_COUNTS = (0, 1, 2, 3, 4, 5, 8)   # SSTs starting in a range: every value must occur somewhere
CLASSES = ("swallowed", "swallowed_at_m", "no_lift", "lift", "sst_in_range", "no_sst_in_range", "ends_at_m",
           "crosses_m", "stream_ends_inside")


def halo_formula(path=cc._SRC):
    """(d, a) of lsmblk_shard_halo_entries: block_size / d + a.  A missing one raises."""
    with open(path) as f:
        m = re.search(r"lsmblk_shard_halo_entries\(uint32_t block_size\)\s*\{\s*return uint64_t\(block_size\) / (\d+) \+ (\d+);",
                      f.read())
    if not m:
        raise RuntimeError(f"lsmblk_shard_halo_entries: no `block_size / D + A` in {path}")
    return int(m.group(1)), int(m.group(2))


HALO = halo_formula()


def halo_entries(bs, halo=HALO):
    return bs // halo[0] + halo[1]


def flevels_formula(path=cc._SRC):
    """shard_flevels' loop condition as written (the restatement below holds for this text only)."""
    with open(path) as f:
        m = re.search(r"uint32_t shard_flevels\(uint32_t sst_cap\) \{\s*uint32_t k = 1;\s*while \((.*?)\) \+\+k;", f.read())
    if not m:
        raise RuntimeError(f"shard_flevels: not found in {path}")
    return m.group(1)


FLEVELS_TEXT = "k < 32 && (1ull << k) < uint64_t(sst_cap) + 1"


def shard_flevels(sst_cap):
    """shard_flevels of lsmblk_compact.hip: the carry counts up to 2^flevels SSTs starting in a range."""
    k = 1
    while k < 32 and (1 << k) < sst_cap + 1:
        k += 1
    return k


# ------------------------------------------------------------------------------- extended streams
@dataclass
class ExtCase:
    name: str
    config: str
    ext: O.KV                 # the range's own m entries, then the halo
    m: int
    last: bool                # LSMBLK_SHARD_LAST
    bs: int
    target: int
    same: np.ndarray = None   # the _ex form: same_as_last_key per ext entry (None: the previous entry's key)

    @property
    def n(self):
        return self.ext.n


def version_stream(bs, nkeys=330):
    """Sorted 7-byte keys of one, two and three versions (ts descending), values of 0 .. bs / 10 bytes, the last
    key of one version; key 30 has a version group longer than a block (info: its first entry, its length)."""
    vmax, glen = bs // 10, bs // 8
    ents, group = [], None
    for i in range(nkeys):
        nv = glen if i == 30 else 1 if i == nkeys - 1 else (1, 2, 1, 3, 2, 1, 1, 3)[i % 8]
        if i == 30:
            group = (len(ents), nv)
        for v in range(nv):
            ents.append((b"s%06d" % (3 * i + 1), 1000 - v, bytes([97 + (i + v) % 26]) * ((i * 7 + v * 3) % (vmax + 1))))
    return O.KV.from_entries(ents), group


def key_changes(kv):
    """Entries whose key differs from the previous entry's (entry 0 left out)."""
    ko, kb = kv.key_off.tolist(), kv.keys.tobytes()
    return [i for i in range(1, kv.n) if kb[ko[i - 1]:ko[i]] != kb[ko[i]:ko[i + 1]]]


def _change_at_or_after(changes, i):
    return next(c for c in changes if c >= i)


def cut(stream, a, m_abs, h):
    """ext = stream[a : m_abs + h): own count m_abs - a, then h halo entries."""
    return O.gather(stream, np.arange(a, m_abs + h)), m_abs - a


def configs(c=C):
    """{name: (block_size, target)}: per block size a target of one block-chain level and one of three."""
    out = {}
    for bs in BLOCK_SIZES:
        t = cc.level_targets(bs, c)
        out[f"bs{bs}-l1"] = (bs, t[1])
        out[f"bs{bs}-l3"] = (bs, t[3])
    out["ex"] = (BLOCK_SIZES[0], cc.level_targets(BLOCK_SIZES[0], c)[1])
    return out


def explicit_same(ext, m):
    """A same_as_last_key array that is not "equal to the previous key": 1 on every 7th real key change, 0
    on every 5th entry inside a key's versions; same[0] == same[m] == 0."""
    changes = set(key_changes(ext))
    same = np.array([0] + [0 if i in changes else 1 for i in range(1, ext.n)], np.uint8)
    flips = [0, 0]
    for q, i in enumerate(sorted(changes)):
        if q % 7 == 3 and i != m:
            same[i] = 1
            flips[0] += 1
    for q, i in enumerate(i for i in range(1, ext.n) if i not in changes):
        if q % 5 == 2 and i != m:
            same[i] = 0
            flips[1] += 1
    assert same[0] == 0 and same[m] == 0 and min(flips) >= 5, flips
    return same


def ext_cases(c=C, halo=HALO):
    """Per configuration two extended streams: `mid` (a full halo, the stream goes on: no LAST) and `tail` (the
    stream's last ~160 entries, a halo of one entry, LAST)."""
    out = []
    for name, (bs, target) in configs(c).items():
        stream, group = version_stream(bs)
        ch = key_changes(stream)
        W = halo_entries(bs, halo)
        m_abs = _change_at_or_after(ch, 430 if name.endswith("l3") else 170 if bs == 64 else 200)
        assert group[0] + group[1] < m_abs and m_abs + W < stream.n
        ext, m = cut(stream, 0, m_abs, W)
        a = _change_at_or_after(ch, stream.n - 165)
        tail, mt = cut(stream, a, stream.n - 1, 1)
        assert stream.n - 1 in ch
        for tag, (e, mm, last) in (("mid", (ext, m, False)), ("tail", (tail, mt, True))):
            out.append(ExtCase(f"{name}-{tag}", name, e, mm, last, bs, target, explicit_same(e, mm) if name == "ex" else None))
    return out


def carry_grid(case):
    """Every carry-in (p, D0): p over [0, m + 3], D0 on both sides of the target."""
    t = case.target
    return [(p, d) for p in range(case.m + 4) for d in (0, 1, t - 1, t, t + case.bs, 1 << 40)]


def oracle_answer(case, p, d0):
    """(rc, segments, (p_out, d_out)) of compact_generate_sst resumed at the carry-in."""
    return O.shard_rotation(case.ext, case.m, case.last, p, d0, case.bs, case.target, same=case.same)


def classify(case, p, d0, ans):
    """The branches of shard_carry_kernel that (p, D0) lands on, from the oracle's answer `ans` and position
    arithmetic: (labels, SSTs starting in the range or None)."""
    rc, seg, (p_out, d_out) = ans
    assert rc == 0, (case.name, p, d0, rc)
    if p >= case.m:
        assert len(seg) == 0 and (p_out, d_out) == (p - case.m, d0)
        return ({"swallowed"} | ({"swallowed_at_m"} if p == case.m else set())), None
    labels = {"no_lift" if d0 >= case.target else "lift"}
    cnt = len(seg) - 2
    assert cnt >= 0 and seg[0] == p and seg[-1] == case.m + p_out
    labels.add("sst_in_range" if cnt else "no_sst_in_range")
    if (p_out, d_out) == (0, 0):
        labels.add("ends_at_m")
    elif d_out == 0:
        assert case.last and p_out == case.n - case.m, (case.name, p, d0, p_out)
        labels.add("stream_ends_inside")
    else:
        labels.add("crosses_m")
    return labels, cnt


def check_config(cases, answers, c=C, halo=HALO):
    """The coverage of one configuration's cases (answers: {(case name, p, D0): oracle answer}): the level count
    its name claims under the constants c, the halo length, every class, and a version group longer than a
    block inside the range.  Returns (classes seen, SST counts seen)."""
    name = cases[0].config
    bs, target = cases[0].bs, cases[0].target
    lv = cc.rot_levels(target, bs, c)
    assert lv == 1 if not name.endswith("l3") else lv >= 3, (name, lv)
    seen, counts = set(), set()
    for case in cases:
        assert (case.config, case.bs, case.target) == (name, bs, target)
        h = case.n - case.m
        assert h == (1 if case.last else halo_entries(bs, halo)) and 150 <= case.n <= 600, (case.name, h, case.n)
        assert case.m in key_changes(case.ext) or case.same is not None
        for p, d0 in carry_grid(case):
            labels, cnt = classify(case, p, d0, answers[(case.name, p, d0)])
            seen |= labels
            if cnt is not None:
                counts.add(cnt)
    assert seen == set(CLASSES), (name, sorted(set(CLASSES) - seen))
    mid = cases[0]
    stream, (g0, glen) = version_stream(bs)
    assert g0 + glen < mid.m and cc.block_end(mid.ext, g0, bs) < g0 + glen   # key_change_after walks past a block start
    nv = np.diff([0] + key_changes(mid.ext)[:200])
    assert {1, 2, 3} <= set(nv.tolist())
    return seen, counts


def all_answers(cases):
    return {(case.name, p, d0): oracle_answer(case, p, d0) for case in cases for p, d0 in carry_grid(case)}


def chain_ranges(case_stream, cuts, bs, target, same=None, halo=HALO):
    """The oracle's answers chained over the ranges [cuts[r], cuts[r + 1]) of a stream, every range's carry-out
    fed to the next: (blocks, SST starts) of the whole stream, as test_shard_oracle.run_chain."""
    W, n, carry = halo_entries(bs, halo), case_stream.n, (0, 0)
    blocks, starts = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        e = min(b + W, n)
        ext = O.gather(case_stream, np.arange(a, e))
        sm = None if same is None else np.concatenate([[0], same[a + 1:e]]).astype(np.uint8)
        rc, seg, cout = O.shard_rotation(ext, b - a, e == n, carry[0], carry[1], bs, target, same=sm)
        assert rc == 0, (a, b, rc)
        if len(seg):
            rc, blk, _ = O.encode_span(ext, seg, bs)
            assert rc == 0
            blocks.append(blk.tobytes())
            starts += [a + int(x) for x in seg[0 if carry[1] == 0 else 1:-1]]
        carry = cout
    return b"".join(blocks), starts


# ------------------------------------------------------------------------------- inputs that must be refused
def error_cases(c=C, halo=HALO):
    """{name: (ExtCase, p, D0)} of the inputs lsmblk_shard_rotation_carry reports LSMBLK_ERR_SEGMENTS for:
      m_inside_versions  the range ends inside a key's versions
      halo_short         no LAST and a halo of one entry where the crossing block takes more (with LAST the
                         same ext is valid: the stream ends inside the SST)
      no_halo            n == m, no LAST, p < m: nothing tells an SST that ends at n from one still open; with
                         the SST far below its target, and with one that reached it
    They are kept out of the carry grid: the oracle has no answer for the last two (ORC_E_INVAL)."""
    bs = BLOCK_SIZES[1]
    l1, l3 = cc.level_targets(bs, c)[1], cc.level_targets(bs, c)[3]
    stream, (g0, glen) = version_stream(bs)
    ch = key_changes(stream)
    W = halo_entries(bs, halo)
    out = {}
    ext, m = cut(stream, 0, g0 + glen // 2, W)
    out["m_inside_versions"] = (ExtCase("m_inside_versions", "err", ext, m, False, bs, l1), 0, 0)
    m_abs = _change_at_or_after(ch, 200)
    ext, m = cut(stream, 0, m_abs, 1)
    out["halo_short"] = (ExtCase("halo_short", "err", ext, m, False, bs, l3), m - 1, 0)
    ext, m = cut(stream, 0, m_abs, 0)
    out["no_halo_open"] = (ExtCase("no_halo_open", "err", ext, m, False, bs, 1 << 30), 0, 0)
    out["no_halo_reached"] = (ExtCase("no_halo_reached", "err", ext, m, False, bs, l1), 0, l1)
    return out


def sst_count_points(case, answers):
    """{c: p} with D0 = target: a carry-in of `case` after which exactly c SSTs start in the range."""
    out = {}
    for p in range(case.m):
        _, cnt = classify(case, p, case.target, answers[(case.name, p, case.target)])
        out.setdefault(cnt, p)
    return out


# ------------------------------------------------------------------------------- range bounds
WM = 600
K16 = b"k" * 16


def bound_runs():
    """Three runs of ~60 keys (run 0 the newest, the last run the two-level merge's lower level b): keys of 1,
    4, 8, 15, 16, 17 and 33 bytes, some proper prefixes of others and some a key followed by zero bytes; one to
    three versions; run 1's timestamps straddle WM, so keys of runs 0 and 1 (and 1 alone) have a newer version
    above the watermark and an older one at or below it; tombstones first in a key's versions; b ends below the
    upper runs' last keys."""
    special = [b"a", b"b", b"k" * 15, K16, b"k" * 17, b"k" * 33, K16 + b"\0", b"ke", b"key", b"key\0", b"key\0\0",
               b"kez", b"m" * 15, b"m" * 15 + b"\x80", b"m" * 16, b"y", b"z"]
    filler = [b"f%03d" % i for i in range(40)] + [b"g%07d" % i for i in range(10)] + [b"n" * 33 + bytes([i]) for i in range(6)]
    keys = sorted(special + filler)
    runs = [[] for _ in range(3)]
    for q, k in enumerate(keys):
        for r in range(3):
            if not ((q + r) % 3 != 0 or q % 5 == 0):
                continue
            if r == 2 and k >= b"n":   # b's last key kb lies below keys of the upper runs
                continue
            for v in range(1 + (q + 2 * r) % 3):
                ts = 900 - 300 * r - 40 * v + q % 7
                tomb = v == 0 and ((r == 2 and q % 4 == 0) or (r == 1 and q % 7 == 0))
                runs[r].append((k, ts, b"" if tomb else b"%d.%d.%d" % (q, r, v)))
    return cc.case_of_runs(runs, wm=WM)


def bound_pairs(case):
    """[(name, lo, hi)] (None: that side unbounded) on every edge of lo <= key < hi."""
    kb = case.runs()[-1][-1][0]
    return [
        ("lo equals a key", K16, None), ("hi equals a key", None, K16),
        ("a key is a proper prefix of lo", b"k" * 17 + b"a", None), ("a key is a proper prefix of hi", None, b"k" * 17 + b"a"),
        ("lo is a proper prefix of a key", b"k" * 20, None), ("hi is a proper prefix of a key", None, b"k" * 20),
        ("lo a key and a prefix of keys, hi a key followed by zero", b"ke", b"key\0"),
        ("lo a key followed by zero that is no key", b"kez\0", None), ("hi of one byte, a key", None, b"b"),
        ("zero-length lo", b"", None), ("zero-length hi", None, b""), ("zero-length lo and hi", b"", b""),
        ("lo equals hi", K16, K16), ("lo above hi", b"m", b"f"), ("both bounds keys", b"f030", K16),
        ("one key in range", b"k" * 33, b"k" * 33 + b"\0"), ("range above every key", b"zz", None),
        ("range below every key", None, b"\0"), ("lo at b's last key", kb, None), ("hi at b's last key", None, kb),
        ("lo just above b's last key", kb + b"\0", None), ("unbounded", None, None),
    ]


def splitter_sets():
    """Consecutive splitters: equal to a key, a proper prefix of a key, a key followed by zero (a key itself, and
    not), and repeated (an empty range)."""
    return [[b"f030", b"key\0", b"kez\0", K16, b"k" * 20, b"m" * 15], [b"", b"a", b"a\0", b"k" * 15, b"k" * 15, b"k" * 17, b"z"]]


def in_bounds(key, lo, hi):
    return (lo is None or lo <= key) and (hi is None or key < hi)


def merged_entries(case, mode, two_end=LSMBLK_TWO_END_IN_RANGE):
    """The merged stream over the whole input: the C oracle's MergeIterator, the newest order, or the two-level
    iterator of oracle/pyref.py.  A two-level range that does not hold b's last key merges as include/lsmblk.h
    words its two_end: LSMBLK_TWO_END_ABOVE "no cut-off in it" (pyref's closed form with an end above every
    key), LSMBLK_TWO_END_BELOW "no a-entry survives" (the same without the upper runs' entries); what differs
    from the single stream lies outside such a range."""
    kv = case.kv
    if mode == TWO:
        if two_end == LSMBLK_TWO_END_IN_RANGE:
            return pyref.two_merge_runs(case.runs())
        uncut = pyref.two_merge_rule(case.runs(), b"\xff" * 64)
        b = set(case.runs()[-1])   # (a key's timestamps differ from run to run: an entry names its run)
        return uncut if two_end == LSMBLK_TWO_END_ABOVE else [e for e in uncut if e in b]
    src = O.merge_runs(kv, case.rs) if mode == RUNS else mn.newest_order(case)
    return [kv.entry(int(i)) for i in src]


def kept_entries(case, mode, bottom):
    """The kept stream of the unrestricted compaction (single stream)."""
    kv = case.kv
    if mode == TWO:
        return [e for e, _ in pyref.compact_rules_trace(pyref.drain(pyref.two_merge_iter(case.runs())), WM, bottom)]
    src = O.merge_runs(kv, case.rs) if mode == RUNS else mn.newest_order(case)
    kept = O.compact(kv, src, WM, bottom, (), 4096, 1 << 20, kept_only=True)["kept"]
    return [kv.entry(int(i)) for i in src[kept]]


def check_bound_cases(case):
    """The run set has the key lengths, prefixes and watermark straddles bound_pairs relies on, and every pair
    sits on the edge its name claims."""
    runs = case.runs()
    keys = sorted({e[0] for r in runs for e in r})
    assert len(runs) == 3 and all(40 <= len({e[0] for e in r}) <= 80 for r in runs), [len(r) for r in runs]
    assert {1, 15, 16, 17, 33} <= {len(k) for k in keys}
    assert sum(1 for a in keys for b in keys if a != b and b.startswith(a)) >= 8
    kb = runs[-1][-1][0]
    assert kb < max(keys) and any(e[0] > kb for e in runs[0])
    ents = [e for r in runs for e in r]
    assert len(set(ents)) == len(ents) and len({(k, ts) for k, ts, _ in ents}) == len(ents)
    single = merged_entries(case, TWO)
    assert set(merged_entries(case, TWO, LSMBLK_TWO_END_BELOW)) < set(single) < set(merged_entries(case, TWO, LSMBLK_TWO_END_ABOVE))
    merged = merged_entries(case, NEWEST)
    straddle = {k for k in keys if any(e[0] == k and e[1] > WM for e in merged) and any(e[0] == k and e[1] <= WM for e in merged)}
    assert len(straddle) >= 10
    for bottom in (False, True):
        for mode in (RUNS, NEWEST, TWO):
            kept, mg = kept_entries(case, mode, bottom), merged_entries(case, mode)
            assert 0 < len(kept) < len(mg)   # the rules cut version groups
    pairs = {name: (lo, hi) for name, lo, hi in bound_pairs(case)}
    ks = set(keys)
    assert pairs["lo equals a key"][0] in ks and pairs["hi equals a key"][1] in ks
    lo = pairs["a key is a proper prefix of lo"][0]
    assert lo not in ks and lo[:-1] in ks and any(k > lo for k in keys if k.startswith(lo[:-1]))
    lo = pairs["lo is a proper prefix of a key"][0]
    assert lo not in ks and any(k.startswith(lo) for k in keys) and any(lo.startswith(k) for k in keys)
    lo, hi = pairs["lo a key and a prefix of keys, hi a key followed by zero"]
    assert lo in ks and hi in ks and hi[:-1] in ks and hi + b"\0" in ks
    assert pairs["lo a key followed by zero that is no key"][0][:-1] in ks and pairs["lo a key followed by zero that is no key"][0] not in ks
    lo, hi = pairs["lo above hi"]
    assert lo > hi and any(hi <= k < lo for k in keys)
    lo, hi = pairs["one key in range"]
    assert [k for k in keys if in_bounds(k, lo, hi)] == [lo]
    for name in ("zero-length hi", "zero-length lo and hi", "lo equals hi", "lo above hi", "range above every key",
                 "range below every key"):
        assert not [k for k in keys if in_bounds(k, *pairs[name])], name
    assert [k for k in keys if in_bounds(k, *pairs["zero-length lo"])] == keys
    # out of range, the watermark rules still cut a version group
    lo, hi = pairs["both bounds keys"]
    kept = kept_entries(case, NEWEST, False)
    assert any(not in_bounds(e[0], lo, hi) and e not in kept for e in merged)
    for sp in splitter_sets():
        assert sp == sorted(sp)
    return keys
