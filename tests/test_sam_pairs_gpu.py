"""The paired SAM formatter on the device (csrc/sam_pair_format.hip behind PairedAligner).

Device against the reference: the two decoded fixtures of the reference's own paired records
(sam_pair_cases.decode_fixture) through PairedAligner.sam_format.  Device against the host, byte for
byte: the fabricated cases, and batches of Reads.synthetic_pairs on the small world at the sizes at
which the kernels take another path (one record pair; 32 records = one workgroup; 34 = past it;
2,050 = past one 2,048-length scan tile; 80 records of 500 bases with 200-byte ids, so that a
workgroup's records pass the 16 KiB LDS window).  The resident chain align -> run_cigars -> run_sam
-> sam() against sam_format_pairs of the same results and the downloaded CIGARs, and its states."""
import numpy as np
import pytest

import snapgpu
from sam_pair_cases import (FIXTURES, decode_fixture, fabricated, small_index, split_lines, synthetic_batch,
                            too_long_batch)

pytestmark = pytest.mark.gpu
EINVAL = r"\(-1\)"


@pytest.fixture(scope="module")
def small(gpu_available):
    """The paired aligner on the index of small.fa (the fixtures' and the fabricated cases' pieces)."""
    index = small_index()
    return index, snapgpu.PairedAligner(index, device=0)


@pytest.fixture(scope="module")
def world(gpu_available, small_world):
    index = small_world["index"]
    return dict(index=index, genome=small_world["genome"], pa=snapgpu.PairedAligner(index, device=0),
                base=snapgpu.BaseAligner(index, maxHitsToConsider=16000, maxK=15, maxSeedsToUse=8, extraSearchDepth=2))


@pytest.mark.parametrize("stem", sorted(FIXTURES))
def test_device_gives_the_reference_records(small, stem):
    index, pa = small
    batch, lines, _ = decode_fixture(stem)
    got = split_lines(pa.sam_format(*batch.args()))
    assert len(got) == len(lines)
    bad = [j for j in range(len(lines)) if got[j] != lines[j]]
    assert not bad, (len(bad), got[bad[0]], lines[bad[0]])


@pytest.mark.parametrize("read_group", ["FASTQ", None, "g" * 300])
def test_fabricated_cases_equal_the_host(small, read_group):
    index, pa = small
    batch, names = fabricated()
    want = split_lines(snapgpu.sam_format_pairs(index, *batch.args(), read_group=read_group))
    got = split_lines(pa.sam_format(*batch.args(), read_group=read_group))
    assert len(got) == len(want)
    for q, name in enumerate(names):
        assert got[2 * q:2 * q + 2] == want[2 * q:2 * q + 2], name
    # and with the ends exchanged (end 1 first wherever its location is the lower one)
    x = batch.exchanged()
    assert pa.sam_format(*x.args(), read_group=read_group) == snapgpu.sam_format_pairs(index, *x.args(), read_group=read_group)


def test_batch_form_refusals(small):
    index, pa = small
    batch, _ = fabricated()
    r0, r1, res, cig = batch.args()
    with pytest.raises(snapgpu.SnapGpuError, match="1024"):
        pa.sam_format(*too_long_batch().args())
    many = snapgpu.Cigars(cig.editDistance.copy(), cig.nOps.copy(), cig.ops.copy())
    many.nOps[7] = snapgpu._ffi.CIGAR_MAX_OPS + 1
    with pytest.raises(snapgpu.SnapGpuError, match="nOps"):
        pa.sam_format(r0, r1, res, many)
    C = snapgpu.C
    used = C.c_uint64()
    short = r1.slice(0, batch.n - 1)
    args = [res.ctypes.data, cig.editDistance.ctypes.data, cig.nOps.ctypes.data, cig.ops.ctypes.data, b"FASTQ"]
    fn = snapgpu.lib().snapgpu_sam_format_pairs_gpu
    assert fn(pa._h, index._h, r0._p, short._p, *args, None, 0, C.byref(used)) == -1
    # the size contract: the bytes needed come back with the refusal, and then suffice
    text = snapgpu.sam_format_pairs(index, r0, r1, res, cig)
    buf = C.create_string_buffer(len(text))
    assert fn(pa._h, index._h, r0._p, r1._p, *args, buf, len(text) - 1, C.byref(used)) == -1 and used.value == len(text)
    assert fn(pa._h, index._h, r0._p, r1._p, *args, buf, len(text), C.byref(used)) == 0 and buf.raw == text


def _chain(w, r0, r1):
    """align -> run_cigars -> run_sam -> sam() on the resident batch, checked against the host formatter
    over the same results and the downloaded CIGARs, and against the batch form -> (results, text)."""
    pa, index = w["pa"], w["index"]
    res = pa.align(r0, r1)
    pa.run_cigars(res)
    pa.run_sam(r0, r1)
    text = pa.sam()
    cig = pa.cigars()
    want = snapgpu._pair_cigars(w["base"], r0, r1, res)   # BaseAligner CIGARs of the same locations
    assert np.array_equal(cig.editDistance, want.editDistance) and np.array_equal(cig.nOps, want.nOps)
    assert np.array_equal(cig.ops, want.ops)
    host = snapgpu.sam_format_pairs(index, r0, r1, res, cig)
    assert len(split_lines(host)) == 2 * r0.n
    assert text == host
    pa.run_sam(r0, r1)   # a second run over the same resident batch
    assert pa.sam() == host
    assert pa.sam_format(r0, r1, res, cig) == host
    return res, host


@pytest.mark.parametrize("clipped", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("n", [1, 16, 17, 1025])
def test_synthetic_pairs_equal_the_host(world, n, clipped):
    r0, r1 = synthetic_batch(world["genome"], n, clipped, seed=31 + n)
    res, host = _chain(world, r0, r1)
    found = res["status"] != snapgpu.NotFound
    if n >= 16:
        assert found.all(axis=1).sum() > n // 4
    if clipped and n == 1025:   # the replaced ends give half-mapped and unmapped pairs, the tails soft clips
        assert (found[:, 0] != found[:, 1]).sum() > 20 and (~found.any(axis=1)).sum() > 5
        assert sum(l.split(b"\t")[5].endswith(b"S") for l in split_lines(host)) > 100
        flags = {int(l.split(b"\t")[1]) & 0xc for l in split_lines(host)}
        assert flags == {0, 4, 8, 12}


def test_records_that_pass_the_lds_window(world):
    """40 pairs of 500-base ends with 200-byte ids: a workgroup's 32 records are some 40 KB of text,
    composed in several 16 KiB windows."""
    r0, r1 = synthetic_batch(world["genome"], 40, False, seed=77, read_length=500, id_length=200)
    _, host = _chain(world, r0, r1)
    lines = split_lines(host)
    assert sum(len(l) for l in lines[:snapgpu.SAM_RECORDS_PER_WORKGROUP]) > 2 * 16384
    assert all(len(l.split(b"\t")[0]) == 198 and len(l.split(b"\t")[9]) == 500 for l in lines)


def test_resident_chain_states(world):
    pa, index = world["pa"], world["index"]
    fresh = snapgpu.PairedAligner(index, device=0)
    r0, r1 = synthetic_batch(world["genome"], 300, False, seed=5)
    s0, s1 = synthetic_batch(world["genome"], 300, True, seed=5)   # the same n, other lengths
    t0, t1 = synthetic_batch(world["genome"], 299, False, seed=5)
    res = np.zeros(300, dtype=snapgpu.PAIR_RESULT_DTYPE)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):   # no batch resident
        fresh.run_cigars(res)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):
        fresh.run_sam(r0, r1)
    res = pa.align(r0, r1)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):   # no CIGAR pass behind it
        pa.run_sam(r0, r1)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):
        pa.cigars()
    assert pa.resident_pairs() == 300 and fresh.resident_pairs() == 0
    for wrong in (res[:299], res[::2], np.concatenate([res, res[:1]]), res.reshape(150, 2)):
        with pytest.raises(ValueError):   # the C call takes no count: one record per resident pair, or refused
            pa.run_cigars(wrong)
    pa.run_cigars(res)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):   # no text yet
        pa.sam()
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):   # another batch: n, then lengths
        pa.run_sam(t0, t1)
    assert (s0.lengths() != r0.lengths()).any()
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):
        pa.run_sam(s0, s1)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):
        pa.run_sam(r0, s1)
    pa.run_sam(r0, r1)
    cig = pa.cigars()
    # an align that follows a run_sam that was not downloaded waits for it and gives the same results
    again = pa.align(r0, r1)
    assert again.tobytes() == res.tobytes()
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):   # the new align made CIGARs and text stale
        pa.sam()
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):
        pa.run_sam(r0, r1)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):
        pa.cigars()
    pa.run_cigars(again)
    pa.run_sam(r0, r1, read_group=None)
    want = snapgpu.sam_format_pairs(index, r0, r1, res, cig, read_group=None)
    assert pa.sam() == want and b"RG:Z:" not in want
    # the batch form leaves the resident rows alone and takes the text buffers
    other = pa.sam_format(s0, s1, pa_results(world, s0, s1), snapgpu.Cigars.empty(600))
    assert other.count(b"\n") == 600
    assert np.array_equal(pa.cigars().ops, cig.ops)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):
        pa.sam()
    pa.run_sam(r0, r1, read_group=None)
    assert pa.sam() == want
    cigar_ms, kernel_ms, download_ms = pa.sam_ms()
    assert cigar_ms > 0 and kernel_ms > 0 and download_ms > 0


def pa_results(world, r0, r1):
    """Records for a batch that is not aligned: every end NotFound."""
    res = np.zeros(r0.n, dtype=snapgpu.PAIR_RESULT_DTYPE)
    res["location"] = 0xFFFFFFFF
    return res
