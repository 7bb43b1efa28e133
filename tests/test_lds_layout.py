"""align_kernel<128>'s LDS layout and the persistent grids.

A CU allocates LDS in units of 1,280 B, so 20 one-wave workgroups are resident together only at 7,680 B
or less each.  Aligners whose score limit (maxK + extraSearchDepth) is at most 16 run pass 1 on 16
Landau-Vishkin rows (7,552 B); the others keep 30 rows.  Every persistent grid is the workgroups that
are resident per CU times the compute units.

No LDS cap changed its value (ELCAP 6, the order window 128, SKCAP / MIRCAP 192), but the tables behind
them moved, so the reads below still end with element counts on both sides of each of them.  They were
chosen with the oracle: of READS_ALL's 20,000 reads it counts 522 / 387 / 319 with 5 / 6 / 7 elements,
14 / 8 / 5 with 127 / 128 / 129 and 27 / 34 / 31 with 191 / 192 / 193.
"""
import numpy as np
import pytest

import snapgpu
from oracle_ffi import mismatches, oracle_align

pytestmark = pytest.mark.gpu

GENOME = dict(total_bases=2_000_000, seed=5, n_contigs=2, n_repeat_families=12, repeat_fraction=0.7)
N_ALL = 20_000
N_READS = 2_000
# element counts just below, at and just above ELCAP, the forced-mode order window and SKCAP / MIRCAP
BOUNDARIES = {"ELCAP": (5, 6, 7), "order window": (127, 128, 129), "SKCAP / MIRCAP": (191, 192, 193)}
PER_COUNT = 40          # reads kept per boundary count
WAVES_PER_CU_128 = 20   # 5 waves per SIMD at 96 VGPRs


@pytest.fixture(scope="module")
def world():
    idx = snapgpu.GenomeIndex.build(snapgpu.Genome.synthetic(**GENOME), 20, 8)   # takes ownership of the genome
    every = snapgpu.Reads.synthetic(snapgpu.Genome.synthetic(**GENOME), N_ALL, seed=99)
    ne = oracle_align(idx, every, snapgpu.default_params())["nElements"]
    keep = []
    for counts in BOUNDARIES.values():
        for c in counts:
            keep += list(np.nonzero(ne == c)[0][:PER_COUNT])
    keep = set(int(i) for i in keep)
    rest = [i for i in range(N_ALL) if i not in keep]
    sel = sorted(list(keep) + rest[:N_READS - len(keep)])
    reads = snapgpu.Reads.from_list([every.get(i) for i in sel])
    return {"index": idx, "reads": reads, "oracle": oracle_align(idx, reads, snapgpu.default_params())}


def _diff(gpu, cpu, bad, k=3):
    return "\n".join(f"read {i}\n  gpu={gpu[i]}\n  cpu={cpu[i]}" for i in bad[:k])


def test_cap_boundaries(gpu_available, world):
    """Reads on each side of every LDS cap, all equal to the oracle."""
    assert world["reads"].n == N_READS
    al = snapgpu.BaseAligner(world["index"])
    gpu = al.AlignReads(world["reads"])
    bad = mismatches(gpu, world["oracle"])
    assert len(bad) == 0, f"{len(bad)} of {len(gpu)} differ\n" + _diff(gpu, world["oracle"], bad)
    for cap, counts in BOUNDARIES.items():
        for c in counts:
            n = int((gpu["nElements"] == c).sum())
            print(f"{cap}: {n} reads with {c} elements")
            assert n >= 1, f"no read with {c} elements ({cap})"


ROW_SETS = [(dict(maxK=14, extraSearchDepth=2), 1), (dict(maxK=15, extraSearchDepth=2), 0),
            (dict(maxK=30, extraSearchDepth=1), 0)]


@pytest.mark.parametrize("kw,short", ROW_SETS, ids=["limit16_short_rows", "limit17_full_rows", "maxK30_full_rows"])
def test_row_capacity(gpu_available, world, kw, short):
    """The same reads at the largest limit of the 16-row kernel, at the smallest of the 30-row kernel and at
    maxK 30: each equals the oracle."""
    al = snapgpu.BaseAligner(world["index"], **kw)
    g = al.debug_grids()
    assert g["shortRows"] == short
    assert (g["lds128"] <= 7680) == bool(short)
    gpu = al.AlignReads(world["reads"])
    cpu = oracle_align(world["index"], world["reads"], al.params)
    bad = mismatches(gpu, cpu)
    assert len(bad) == 0, f"{kw}: {len(bad)} of {len(gpu)} differ\n" + _diff(gpu, cpu, bad)


def _lds_fit(g, lds):
    unit = g["ldsUnit"]
    return g["ldsPerCU"] // ((lds + unit - 1) // unit * unit)


def _check_grids(g, cap=None):
    cus = g["computeUnits"]
    assert cus > 0 and g["ldsUnit"] == 1280
    for k in ("128", "256", "512", "Simple", "Cigar"):
        assert g["perCU" + k] >= 1
        if cap is not None:
            assert g["perCU" + k] <= cap
    want128 = min(WAVES_PER_CU_128, _lds_fit(g, g["lds128"]))
    assert g["perCU128"] == (want128 if cap is None else min(want128, cap))
    assert g["grid128"] == g["perCU128"] * cus
    assert g["grid256"] == min(g["perCU256"] * cus, g["grid128"])   # passes 2 and 3 reuse pass 1's arenas
    assert g["grid512"] == min(g["perCU512"] * cus, g["grid128"])
    assert g["gridSimple"] == g["perCUSimple"] * cus
    assert g["gridCigar"] == g["perCUCigar"] * cus


def test_grid_sizes(gpu_available, world, monkeypatch):
    """Every persistent grid is the resident workgroups per CU times the compute units; the 16-row kernel
    keeps 20 waves per CU resident, the 30-row kernel 18; SNAPGPU_WAVES_PER_CU shrinks the grids."""
    g = snapgpu.BaseAligner(world["index"]).debug_grids()
    print(g)
    _check_grids(g)
    assert g["shortRows"] == 1 and g["perCU128"] == 20
    full = snapgpu.BaseAligner(world["index"], maxK=15, extraSearchDepth=2).debug_grids()
    _check_grids(full)
    assert full["shortRows"] == 0 and full["perCU128"] == 18
    monkeypatch.setenv("SNAPGPU_WAVES_PER_CU", "3")
    few = snapgpu.BaseAligner(world["index"]).debug_grids()
    _check_grids(few, cap=3)
    assert few["grid128"] == 3 * few["computeUnits"]


def test_paired_grid_sizes(gpu_available, world):
    g = snapgpu.PairedAligner(world["index"]).debug_grids()
    print(g)
    cus = g["computeUnits"]
    assert cus > 0 and min(g["perCU128"], g["perCU256"], g["perCU512"]) >= 1
    assert g["grid128"] == g["perCU128"] * cus
    assert g["grid256"] == min(g["perCU256"] * cus, g["grid128"])
    assert g["grid512"] == g["perCU512"] * cus
    assert 1 <= g["gridPools"] <= g["grid512"]
