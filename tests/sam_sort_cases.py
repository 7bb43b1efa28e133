"""Inputs shared by test_sam_sort_keys.py (CPU) and test_sam_gpu_sorted.py: the six-contig genome
whose names exercise the sort key's name rules, and the key order itself."""
import numpy as np

import snapgpu

# two pieces named chrA (the host sorter's name -> offset map keeps the first), a name that begins
# with '*' and an empty name (both read as "no location"), and plain names around them
SIX_NAMES = ("chrA", "chrB", "chrA", "*star", "", "chrC")


def six_contig_index(tmp_dir):
    """GenomeIndex over a FASTA of SIX_NAMES, 3,000 random bases each, padding 500."""
    rng = np.random.default_rng(61)
    path = tmp_dir / "six.fa"
    with open(path, "w") as f:
        for name in SIX_NAMES:
            seq = "".join(rng.choice(list("ACGT"), size=3000))
            f.write(f">{name}\n" + "\n".join(seq[i:i + 60] for i in range(0, 3000, 60)) + "\n")
    idx = snapgpu.GenomeIndex.build(snapgpu.Genome.from_fasta(str(path), 500), 20, 8)
    assert idx.view().nPieces == len(SIX_NAMES)
    return idx


def key_order(idx, results):
    """The order of coordinate-sorted output: the stable argsort of the records' sort keys."""
    return np.argsort(snapgpu.sam_sort_keys(idx, results), kind="stable").astype(np.uint32)


def reorder(text, order):
    """The lines of `text` (one per record) in `order` -> bytes."""
    lines = text.splitlines(keepends=True)
    assert len(lines) == len(order)
    return b"".join(lines[int(i)] for i in order)
