"""The paired BAM encoder on the device (csrc/bam_pair_format.hip behind PairedAligner).

Device against the reference: the four decoded fixtures of the reference's own paired BAM records
(bam_pair_cases.fixture_runs) through PairedAligner.bam_format, every record.  Device against the
host, byte for byte: the fabricated cases, and batches of Reads.synthetic_pairs on the small world
through the resident chain align -> run_cigars -> run_bam -> bam() at the sizes at which the kernels
take another path (one pair; 32 records = one workgroup of the write pass; 34 = past it; 2,050 = past
one 2,048-value scan tile; 80 records of 500 bases with 200-byte ids, so that a workgroup's records
pass the 16 KiB LDS window).  The NM carry into a second scan tile, the coordinate order, and the
chain's states."""
import numpy as np
import pytest

import snapgpu
from bam_pair_cases import VARIANTS, bam_fabricated, fixture_runs, record_fields, split_records, unmapped_run_batch
from sam_pair_cases import small_index, synthetic_batch, too_long_batch

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
    return dict(index=index, genome=small_world["genome"], pa=snapgpu.PairedAligner(index, device=0))


@pytest.mark.parametrize("stem,variant", VARIANTS)
def test_device_gives_the_reference_records(small, stem, variant):
    index, pa = small
    records = 0
    for run in fixture_runs(stem, variant):
        carry = 0
        for batch, want in run:
            got, carry = pa.bam_format(*batch.args(), nm_carry=carry)
            g, w = split_records(got), split_records(want)
            assert len(g) == len(w)
            bad = [j for j in range(len(w)) if g[j] != w[j]]
            assert not bad, (len(bad), record_fields(g[bad[0]]), record_fields(w[bad[0]]))
            records += len(w)
            assert carry == record_fields(w[-1])["nm"]
    assert records == {"rna": 5998, "rna150": 4000}[stem]


@pytest.mark.parametrize("read_group", ["FASTQ", None, "g" * 300])
def test_fabricated_cases_equal_the_host(small, read_group):
    index, pa = small
    batch, names = bam_fabricated()
    want, want_carry = snapgpu.bam_format_pairs(index, *batch.args(), read_group=read_group, nm_carry=7)
    got, carry = pa.bam_format(*batch.args(), read_group=read_group, nm_carry=7)
    g, w = split_records(got), split_records(want)
    assert len(g) == len(w)
    for q, name in enumerate(names):
        assert g[2 * q:2 * q + 2] == w[2 * q:2 * q + 2], name
    assert carry == want_carry
    # and with the ends exchanged (end 1 first wherever its location is the lower one)
    x = bam_fabricated(False)[0].exchanged()
    assert pa.bam_format(*x.args(), read_group=read_group) == snapgpu.bam_format_pairs(index, *x.args(), read_group=read_group)


def test_batch_form_refusals(small):
    index, pa = small
    batch, _ = bam_fabricated()
    r0, r1, res, cig = batch.args()
    with pytest.raises(snapgpu.SnapGpuError, match="1024"):
        pa.bam_format(*too_long_batch().args())
    with pytest.raises(snapgpu.SnapGpuError, match="254"):   # exchanged: the longest ids keep "/2" "/1"
        pa.bam_format(*batch.exchanged().args())
    many = snapgpu.Cigars(cig.editDistance.copy(), cig.nOps.copy(), cig.ops.copy())
    many.nOps[7] = snapgpu._ffi.CIGAR_MAX_OPS + 1
    with pytest.raises(snapgpu.SnapGpuError, match="nOps"):
        pa.bam_format(r0, r1, res, many)
    C = snapgpu.C
    used, carry = C.c_uint64(), C.c_int32()
    short = r1.slice(0, batch.n - 1)
    args = [res.ctypes.data, cig.editDistance.ctypes.data, cig.nOps.ctypes.data, cig.ops.ctypes.data, b"FASTQ", 0, C.byref(carry)]
    fn = snapgpu.lib().snapgpu_bam_format_pairs_gpu
    assert fn(pa._h, index._h, r0._p, short._p, *args, None, 0, C.byref(used), 0, None) == -1
    # the size contract: the bytes needed come back with the refusal, and then suffice
    raw, _ = snapgpu.bam_format_pairs(index, r0, r1, res, cig)
    buf = C.create_string_buffer(len(raw))
    assert fn(pa._h, index._h, r0._p, r1._p, *args, buf, len(raw) - 1, C.byref(used), 0, None) == -1 and used.value == len(raw)
    assert fn(pa._h, index._h, r0._p, r1._p, *args, buf, len(raw), C.byref(used), 0, None) == 0 and buf.raw == raw


def _chain(w, r0, r1, nm_carry=0):
    """align -> run_cigars -> run_bam -> bam() on the resident batch, checked against the host encoder
    over the same results and the downloaded CIGARs, and against the batch form -> (results, cigars, records)."""
    pa, index = w["pa"], w["index"]
    res = pa.align(r0, r1)
    pa.run_cigars(res)
    pa.run_bam(r0, r1, nm_carry=nm_carry)
    raw = pa.bam()
    cig = pa.cigars()
    host, host_carry = snapgpu.bam_format_pairs(index, r0, r1, res, cig, nm_carry=nm_carry)
    assert len(split_records(host)) == 2 * r0.n
    assert raw == host and pa.bam_nm_carry() == host_carry
    pa.run_bam(r0, r1, nm_carry=nm_carry)   # a second run over the same resident batch
    assert pa.bam() == host
    assert pa.bam_format(r0, r1, res, cig, nm_carry=nm_carry) == (host, host_carry)
    return res, cig, host


@pytest.mark.parametrize("clipped", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("n", [1, 16, 17, 1025])
def test_synthetic_pairs_equal_the_host(world, n, clipped):
    r0, r1 = synthetic_batch(world["genome"], n, clipped, seed=31 + n)
    res, _, host = _chain(world, r0, r1, nm_carry=n % 5)
    found = res["status"] != snapgpu.NotFound
    if n >= 16:
        assert found.all(axis=1).sum() > n // 4
    if clipped and n == 1025:   # the replaced ends give half-mapped and unmapped pairs, the tails soft clips
        assert (found[:, 0] != found[:, 1]).sum() > 20 and (~found.any(axis=1)).sum() > 5
        f = [record_fields(r) for r in split_records(host)]
        assert sum(1 for x in f if x["ops"] and x["ops"][-1] & 15 == 4) > 100
        assert {x["flag"] & 0xc for x in f} == {0, 4, 8, 12}
        assert sum(1 for x in f if x["flag"] & 0x4 and x["nm"] > 0) > 5   # carried NM values


def test_nm_carry_across_a_scan_tile(small):
    """Pairs 1,000 - 1,060 unmapped on both ends: records 2,000 - 2,119 repeat the NM of record 1,999,
    which enters the second 2,048-value tile from the first.  And a batch that begins with 80 such
    records: they repeat the carry-in."""
    index, pa = small
    batch = unmapped_run_batch(1100, 1000, 1060)
    want, want_carry = snapgpu.bam_format_pairs(index, *batch.args(), nm_carry=3)
    got, carry = pa.bam_format(*batch.args(), nm_carry=3)
    assert got == want and carry == want_carry
    nm = [record_fields(r)["nm"] for r in split_records(got)]
    assert nm[2000:2120] == [nm[1999]] * 120 and nm[1999] == 7 + 999 % 50 + 1 and nm[2120] != nm[1999]
    assert snapgpu.SAM_SCAN_TILE == 2048
    batch = unmapped_run_batch(100, 0, 40)
    want, want_carry = snapgpu.bam_format_pairs(index, *batch.args(), nm_carry=7)
    got, carry = pa.bam_format(*batch.args(), nm_carry=7)
    assert got == want and carry == want_carry
    assert [record_fields(r)["nm"] for r in split_records(got)][:81] == [7] * 80 + [7 + 40]
    # every pair unmapped: the carry-in comes out again
    batch = unmapped_run_batch(30, 0, 30)
    got, carry = pa.bam_format(*batch.args(), nm_carry=-9)
    assert carry == -9 and got == snapgpu.bam_format_pairs(index, *batch.args(), nm_carry=-9)[0]


def test_records_that_pass_the_lds_window(world):
    """40 pairs of 500-base ends with 200-byte ids: a workgroup's 32 records are some 31 KB,
    composed in several 16 KiB windows."""
    r0, r1 = synthetic_batch(world["genome"], 40, False, seed=77, read_length=500, id_length=200)
    _, _, host = _chain(world, r0, r1)
    recs = split_records(host)
    assert sum(len(r) for r in recs[:snapgpu.SAM_RECORDS_PER_WORKGROUP]) > 16384 + 8192
    f = [record_fields(r) for r in recs]
    assert all(len(x["name"]) == 198 and x["l_seq"] == 500 for x in f)


def _sorted_want(index, res, raw):
    keys = snapgpu.bam_pair_sort_keys(index, res)
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    recs = split_records(raw)
    return order, b"".join(recs[j] for j in order), keys


@pytest.mark.parametrize("n", [17, 1025])
def test_sorted_resident_records(world, n):
    pa, index = world["pa"], world["index"]
    r0, r1 = synthetic_batch(world["genome"], n, True, seed=131 + n)
    res = pa.align(r0, r1)
    pa.run_cigars(res)
    pa.run_bam(r0, r1, nm_carry=2)
    unsorted = pa.bam()
    carry = pa.bam_nm_carry()
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):   # the last call was not a sorted one
        pa.bam_order()
    pa.run_bam(r0, r1, sorted_output=True, nm_carry=2)
    got = pa.bam()
    order, want, keys = _sorted_want(index, res, unsorted)
    assert np.array_equal(pa.bam_order(), order)
    assert got == want
    assert pa.bam_nm_carry() == carry   # the NM of the last record in write order, not of the last slot
    assert len(np.unique(keys)) < len(keys)   # unmapped ends sort with their mates: equal keys
    cig = pa.cigars()
    out = np.zeros(2 * n, dtype=np.uint32)
    assert pa.bam_format(r0, r1, res, cig, nm_carry=2, sorted_output=True, order=out) == (want, carry)
    assert np.array_equal(out, order)


def test_sorted_output_is_stable(small):
    """600 records on five locations per end and 120 without any: equal keys keep write order, and the
    NM carry has run over write order before the sort."""
    index, pa = small
    batch = unmapped_run_batch(300, 100, 160, distinct=5)
    unsorted, carry = snapgpu.bam_format_pairs(index, *batch.args(), nm_carry=1)
    order, want, keys = _sorted_want(index, batch.results, unsorted)
    assert len(np.unique(keys)) == 11
    out = np.zeros(600, dtype=np.uint32)
    assert pa.bam_format(*batch.args(), nm_carry=1, sorted_output=True, order=out) == (want, carry)
    assert np.array_equal(out, order)
    with pytest.raises(ValueError):
        pa.bam_format(*batch.args(), order=out)


def test_resident_chain_states(world):
    pa, index = world["pa"], world["index"]
    fresh = snapgpu.PairedAligner(index, device=0)
    r0, r1 = synthetic_batch(world["genome"], 300, False, seed=5)
    s0, s1 = synthetic_batch(world["genome"], 300, True, seed=5)   # the same n, other lengths
    t0, t1 = synthetic_batch(world["genome"], 299, False, seed=5)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):   # no batch resident
        fresh.run_bam(r0, r1)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):
        fresh.bam()
    res = pa.align(r0, r1)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):   # no CIGAR pass behind it
        pa.run_bam(r0, r1)
    pa.run_cigars(res)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):   # no records yet
        pa.bam()
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):   # another batch: n, then lengths
        pa.run_bam(t0, t1)
    assert (s0.lengths() != r0.lengths()).any()
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):
        pa.run_bam(s0, s1)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):
        pa.run_bam(r0, s1)
    # run_sam and run_bam on one batch each return their own bytes, whichever ran last
    pa.run_sam(r0, r1)
    pa.run_bam(r0, r1, nm_carry=4)
    cig = pa.cigars()
    text = snapgpu.sam_format_pairs(index, r0, r1, res, cig)
    records, carry = snapgpu.bam_format_pairs(index, r0, r1, res, cig, nm_carry=4)
    assert pa.sam() == text and pa.bam() == records and pa.bam_nm_carry() == carry
    pa.run_sam(r0, r1, read_group=None)
    assert pa.bam() == records
    assert pa.sam() == snapgpu.sam_format_pairs(index, r0, r1, res, cig, read_group=None)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):   # an unsorted call
        pa.bam_order()
    # an align that follows a run_bam that was not downloaded waits for it and gives the same results
    pa.run_bam(r0, r1, sorted_output=True)
    again = pa.align(r0, r1)
    assert again.tobytes() == res.tobytes()
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):   # the new align made CIGARs and records stale
        pa.bam()
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):
        pa.bam_order()
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):
        pa.run_bam(r0, r1)
    pa.run_cigars(again)
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):   # new CIGARs: the records have to be made again
        pa.bam()
    pa.run_bam(r0, r1, read_group=None, nm_carry=4)
    want, _ = snapgpu.bam_format_pairs(index, r0, r1, res, cig, read_group=None, nm_carry=4)
    assert pa.bam() == want and b"RGZ" not in want
    # the batch form leaves the resident rows and the text alone and takes the record buffers
    pa.run_sam(r0, r1)
    none = np.zeros(300, dtype=snapgpu.PAIR_RESULT_DTYPE)
    none["location"] = 0xFFFFFFFF
    other, other_carry = pa.bam_format(s0, s1, none, snapgpu.Cigars.empty(600), nm_carry=11)
    assert len(split_records(other)) == 600 and other_carry == 11
    assert np.array_equal(pa.cigars().ops, cig.ops) and pa.sam() == text
    with pytest.raises(snapgpu.SnapGpuError, match=EINVAL):
        pa.bam()
    pa.run_bam(r0, r1, read_group=None, nm_carry=4)
    assert pa.bam() == want
    kernel_ms, download_ms = pa.bam_ms()
    assert kernel_ms > 0 and download_ms > 0
