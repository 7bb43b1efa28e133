"""The CPU index builder gives one image whatever its thread count: the GPU builder
(test_index_build_gpu.py) is compared against a single deterministic reference."""
import snapgpu
from index_image import assert_same_index


def test_cpu_build_identical_across_thread_counts(tmp_path):
    def g():
        return snapgpu.Genome.synthetic(1_000_000, seed=2121, n_contigs=3, n_repeat_families=60)
    a = snapgpu.GenomeIndex.build(g(), 20, 1, device=None)
    b = snapgpu.GenomeIndex.build(g(), 20, 8, device=None)
    assert_same_index(a, b, tmp_path)
