"""The SAM line shared by host and device (csrc/sam_line.h), on the CPU: the exact length of every
line, and the writer the device write pass runs per wave here run on one host thread, against the
host formatter snapgpu.sam_format (itself pinned to the reference writer in test_cigar.py)."""
import os
import re

import numpy as np
import pytest

import snapgpu
from sam_cases import READ_GROUPS, clipped_case, fabricated_case, small_case, small_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def idx():
    return small_index()


@pytest.fixture(scope="module")
def fabricated(idx):
    return fabricated_case(idx)


def _line_lengths(text):
    ends = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
    return np.diff(np.concatenate([[-1], ends])).astype(np.uint32)


def _check(idx, case, read_group="FASTQ"):
    reads, ids, res, cig, clip = case
    want = snapgpu.sam_format(idx, reads, ids, res, cig, read_group=read_group, clip=clip)
    got = snapgpu.sam_line_lengths(idx, reads, ids, res, cig, read_group=read_group, clip=clip)
    assert got.dtype == np.uint32 and len(got) == reads.n
    assert int(got.sum(dtype=np.uint64)) == len(want)
    # no byte of a line is a newline but its last, so the line ends give the host formatter's lengths
    lens = _line_lengths(want)
    assert len(lens) == reads.n
    bad = np.flatnonzero(lens != got)
    assert bad.size == 0, f"{bad.size} lengths differ, first {bad[:5]}: {got[bad[:5]]} vs {lens[bad[:5]]}"
    text = snapgpu._sam_line_write(idx, reads, ids, res, cig, read_group=read_group, clip=clip)
    assert text == want


@pytest.mark.parametrize("use_m", [0, 1])
def test_line_lengths_small_reads(idx, use_m):
    """The 2,225 small_reads.fq reads with the reference's records and oracle CIGARs."""
    _check(idx, small_case(idx, use_m))


@pytest.mark.parametrize("use_m", [0, 1])
def test_line_lengths_clipped(idx, use_m):
    """reads.clip(3), oracle records: soft clips, unclipped SEQ / QUAL."""
    case = clipped_case(idx, use_m)
    assert (case[4][1] != case[0].lengths()).sum() > 20   # clipping exercised
    _check(idx, case)


@pytest.mark.parametrize("read_group", READ_GROUPS)
def test_line_lengths_fabricated(idx, fabricated, read_group):
    """5,000 fabricated records that reach every branch of the line (sam_cases.fabricated_case)."""
    _check(idx, fabricated, read_group)


def test_line_lengths_rejects_what_the_formatter_rejects(idx):
    reads = snapgpu.Reads.from_list([("A" * 1025, "I" * 1025)])
    res = np.zeros(1, dtype=snapgpu.RESULT_DTYPE)
    with pytest.raises(snapgpu.SnapGpuError, match="1024"):
        snapgpu.sam_line_lengths(idx, reads, ["r"], res, snapgpu.Cigars.empty(1))
    empty = snapgpu.Reads.from_list([])
    assert len(snapgpu.sam_line_lengths(idx, empty, [], np.zeros(0, dtype=snapgpu.RESULT_DTYPE),
                                        snapgpu.Cigars.empty(0))) == 0


def test_python_mirrors_the_kernels_work_split():
    """snapgpu.SAM_RECORDS_PER_WORKGROUP / SAM_SCAN_TILE (the batch sizes test_sam_gpu.py brackets)
    are the constants the kernels are built with."""
    h = open(os.path.join(ROOT, "snap-rnaseq_amd", "csrc", "sam_format.h")).read()
    val = lambda name: int(re.search(r"constexpr uint32_t %s = (\d+);" % name, h).group(1))
    assert val("kRecsPerGroup") == snapgpu.SAM_RECORDS_PER_WORKGROUP
    assert val("kScanTile") == snapgpu.SAM_SCAN_TILE
