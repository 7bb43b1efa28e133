"""The scoring pass as align_kernel<128> / <256> run it, unit-tested on the device: lv_pass_kernel
(snapgpu.lv_pass_batch) makes lv_pass' calls -- the forward lv_group<1, GS, NW, UNIFORM_K>, the reverse
lv_group<-1, GS, NW> with a limit k - e1 per lane group under the row bound kmax2 -- then pass_apply's gok
packing and lv_prob_groups, with every lane group of a wave holding a different candidate.  The reference is the
oracle's LandauVishkin (oracle_lv, pinned to the reference's vectors by test_oracle_golden.py) called as
BaseAligner::score calls it, on the test's own genome bytes.  Distances and netIndel must be equal, both
probabilities equal as IEEE-754 bit patterns.

The cases (tests/lv_cases.py) are checked by the oracle alone for what they cover (test_pass_cases_cover, no
GPU): the GPU test can only be as strong as that."""
import functools
import struct

import pytest

import lv_cases
import snapgpu

COMBOS = [(gs, nw) for gs in (8, 16, 32, 64) for nw in (2, 4)]
ORACLE_CALLS_MAX = 20_000


@functools.lru_cache(maxsize=None)
def _cases(gs, nw):
    passes = lv_cases.pass_cases(gs, nw)
    return passes, [lv_cases.expected_pass(p) for p in passes]


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


@pytest.mark.parametrize("gs,nw", COMBOS)
def test_pass_cases_cover(gs, nw):
    passes, exp = _cases(gs, nw)
    gn = 64 // gs
    ks = [k for k in lv_cases.KS if lv_cases.group_size(k) == gs]
    assert {p["k"] for p in passes} == set(ks)
    assert {len(p["read"]) for p in passes} == set(lv_cases.NS[nw])
    assert {p["seedLen"] for p in passes} == {16, 20}
    assert {len(p["cands"]) for p in passes} >= {gn, 1, max(1, gn - 1)}
    for p in passes:
        assert lv_cases.group_size(p["k"]) == gs and len(p["cands"]) <= gn
        n = len(p["read"])
        assert all(ord("!") <= q <= ord("M") for q in p["quals"])
        for c in p["cands"]:
            s, t = c["s"], c["s"] + p["seedLen"]
            # the bytes either call may look at are the test's: MAX_K + 2 before position 0, 2 past glen
            assert c["before"] >= lv_cases.MAX_K + 2 and len(c["genome"]) - c["before"] >= max(c["glen"], n) + 34
            assert 0 <= s and t <= n and t <= c["glen"] and n - lv_cases.MAX_K <= c["glen"] <= n + lv_cases.MAX_K
    calls = sum(1 + (e[0] >= 0) for p, ex in zip(passes, exp) for c, e in zip(p["cands"], ex) if c["act"])
    assert calls <= ORACLE_CALLS_MAX, calls
    cands = [(p, c, e) for p, ex in zip(passes, exp) for c, e in zip(p["cands"], ex)]
    assert any(c["s"] == 0 for _, c, _ in cands) and any(c["s"] == 1 for _, c, _ in cands)
    assert any(c["s"] == len(p["read"]) - p["seedLen"] for p, c, _ in cands)
    assert {c["dir"] for _, c, _ in cands} == {0, 1}
    assert sum(1 for _, c, _ in cands if not c["act"]) >= 10
    assert sum(1 for p, c, _ in cands if c["glen"] < len(p["read"]) + lv_cases.MAX_K) >= 10
    assert sum(1 for p, _, _ in cands if b"N" in p["read"]) >= 10
    assert sum(1 for _, c, _ in cands if b"n" in c["genome"]) >= 10
    # exact match, success at exactly k, e1 = k (k2 = 0), failure: each often, and within single passes together
    kmax = max(ks)
    if kmax > 0:
        assert sum(1 for p, _, e in cands if e[0] >= 0 and e[1] >= 0 and e[0] + e[1] == p["k"] and p["k"] > 0) >= 20
        assert sum(1 for p, _, e in cands if e[0] == p["k"] and e[1] == 0 and p["k"] > 0) >= 10
    assert sum(1 for _, _, e in cands if e[0] == 0 and e[1] == 0) >= 20
    if gn > 1:
        mixed = sum(1 for ex in exp if any(e[0] >= 0 and e[1] >= 0 for e in ex) and any(e[0] < 0 for e in ex)
                    and len({e[0] for e in ex}) >= min(3, gn))
        assert mixed >= 20, mixed
    cov = lv_cases.coverage(passes, exp)
    for d in "fr":
        v = cov[d]
        for dist in range(0, min(kmax, gs // 2 - 1) + 1):
            assert v["dist"].get(dist, 0) >= 20, (d, dist, v["dist"])
        assert v["fail"] >= 20, (d, v["fail"])
        for gi in range(gn):
            assert v["group"].get(gi, 0) >= 10, (d, gi, v["group"])
        for kind in lv_cases.INDEL_KINDS:
            assert v["kinds"].get(kind, 0) >= 10, (d, kind, v["kinds"])


@pytest.mark.gpu
@pytest.mark.parametrize("gs,nw", COMBOS)
def test_gpu_lv_pass_matches_oracle(gpu_available, gs, nw):
    passes, exp = _cases(gs, nw)
    got = snapgpu.lv_pass_batch(passes, nw=nw)   # one launch, one wave per pass
    bad = []
    for pi, (p, ex, gt) in enumerate(zip(passes, exp, got)):
        for gi, ((e1, e2, p1, p2, net), (g1, g2, q1, q2, gnet)) in enumerate(zip(ex, gt)):
            ok = (g1, g2) == (e1, e2)
            if ok and e1 >= 0 and e2 >= 0:
                ok = gnet == net and _bits(q1) == _bits(p1) and _bits(q2) == _bits(p2)
            if not ok:
                c = p["cands"][gi]
                bad.append((pi, gi, p["k"], len(p["read"]), c["s"], c["dir"], c["recipe"]["kind"],
                            (e1, e2, net, p1.hex(), p2.hex()), (g1, g2, gnet, q1.hex(), q2.hex())))
    assert not bad, f"{len(bad)} candidates differ from the oracle, first: {bad[:3]}"
