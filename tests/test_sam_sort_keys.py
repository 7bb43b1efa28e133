"""The coordinate-sort key of a record (csrc/sam_line.h sortKey, snapgpu_sam_sort_keys) against the
host sorter, which parses the same key back out of the finished line (samSortKey, csrc/host/sam.cpp):
a stable argsort of the keys, applied to the host formatter's lines, is snapgpu_sam_sort_records'
output byte for byte.  No GPU."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import snapgpu
from sam_cases import G, READ_GROUPS, fabricated_case, small_case, small_index
from sam_sort_cases import SIX_NAMES, key_order, reorder, six_contig_index


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    return {"small": small_index(), "six": six_contig_index(tmp_path_factory.mktemp("six"))}


@pytest.mark.parametrize("read_group", READ_GROUPS)
@pytest.mark.parametrize("genome", ["small", "six"])
def test_key_order_is_the_host_sorters(genomes, genome, read_group):
    idx = genomes[genome]
    reads, ids, res, cig, _ = fabricated_case(idx)
    text = snapgpu.sam_format(idx, reads, ids, res, cig, read_group=read_group)
    order = key_order(idx, res)
    assert reorder(text, order) == snapgpu.sam_sort_records(idx, text)
    assert not np.array_equal(order, np.arange(reads.n))   # the order did change


def test_name_rules_of_the_key(genomes):
    """One record at base 7 of every piece of the six-contig genome, and the three kinds without a
    location: the second chrA sorts with the first one's offset, '*star' and the empty name give
    0xffffffff."""
    idx = genomes["six"]
    v = idx.view()
    piece = [int(x) for x in C.cast(v.pieceOffsets, C.POINTER(C.c_uint32))[:v.nPieces]]
    res = np.zeros(len(piece) + 3, dtype=snapgpu.RESULT_DTYPE)
    res["result"] = snapgpu.SingleHit
    res["location"][:len(piece)] = np.array(piece, dtype=np.uint32) + 7
    res["location"][len(piece)] = 0xFFFFFFFF            # no location
    res["location"][len(piece) + 1] = 3                 # before the first piece
    res["location"][len(piece) + 2] = piece[1] + 9      # a location, but NotFound
    res["result"][len(piece) + 2] = snapgpu.NotFound
    keys = snapgpu.sam_sort_keys(idx, res)
    want = [piece[SIX_NAMES.index(name)] + 7 if name and not name.startswith("*") else 0xFFFFFFFF for name in SIX_NAMES]
    assert keys.tolist() == want + [0xFFFFFFFF] * 3
    assert snapgpu.sam_sort_keys(idx, res[:0]).shape == (0,)


@pytest.mark.parametrize("use_m", [0, 1])
def test_reference_records_sorted_through_the_keys(genomes, use_m):
    """The reference writer's own lines (expected_small.sam.gz) in the key order of its records."""
    idx = genomes["small"]
    _, _, res, _, _ = small_case(idx, use_m)
    lines = gzip.open(os.path.join(G, "expected_small.sam.gz"), "rb").read().splitlines(keepends=True)[use_m::2]
    text = b"".join(lines)
    order = key_order(idx, res)
    assert reorder(text, order) == snapgpu.sam_sort_records(idx, text)
    assert not np.array_equal(order, np.arange(len(res)))
