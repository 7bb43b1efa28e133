"""The .bai index built on the GPU (csrc/bai.hip: field pass, chunk heads, sort, counts, linear index, write,
check): byte-identical to the host model (snapgpu.bai_build), which test_bai_model.py holds to the format's
restatement and to an independent reader.  Every expected value here comes from the model."""
import gzip

import numpy as np
import pytest

import snapgpu
from bai_cases import brute_force, fabricated, parse_bai, query, rec_fields, split

pytestmark = pytest.mark.gpu

SLICES = (0, 1, 5, 33, 300)


@pytest.fixture(scope="module")
def world(gpu_available, small_world):
    """small_world's 4,000 reads aligned once on the device, and one aligner; never modified."""
    idx, reads = small_world["index"], small_world["reads"]
    al = snapgpu.BaseAligner(idx)
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars()
    ids = [b"read_%d extra" % i for i in range(reads.n)]
    return dict(idx=idx, reads=reads, ids=ids, aligner=al, dev=dev)


def _same(got, want, what=""):
    if got != want:
        first = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
        pytest.fail(f"{what}: {len(got)} vs {len(want)} bytes, first difference at byte {first}")


def _aligned(al, reads):
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars()
    return dev


def _sorted_records(world, n, start=0):
    """The sorted BAM records of reads [start, start + n), from the device."""
    if n == 0:
        return b""
    reads = world["reads"].slice(start, n)
    dev = _aligned(world["aligner"], reads)
    dev.run_bam(reads, ids=world["ids"][start:start + n], sorted_output=True)
    return dev.bam()


@pytest.mark.parametrize("off", [0, 1234])
def test_resident_chain(world, off):
    dev, reads, ids = world["dev"], world["reads"], world["ids"]
    dev.run_bam(reads, ids=ids, sorted_output=True)
    dev.run_bgzf()
    dev.run_bai(off)
    got = dev.bai()
    raw, z = dev.bam(), dev.bgzf()               # still the records and the members, after the index
    assert len(raw) > 10 * 0xff00 and gzip.decompress(z) == raw
    _same(got, snapgpu.bai_build(raw, z, 3, off))
    assert {rec_fields(r)["ref"] for r in split(raw)} >= {0, 1, 2}
    _same(dev.bai(), got)                         # the same bytes again
    k, d = world["aligner"].bai_ms()
    assert k > 0 and d > 0


def test_resident_chain_without_a_host_batch(world, tmp_path):
    path = tmp_path / "reads.fq"
    world["reads"].write_fastq(path)
    dev = world["aligner"].upload_fastq(path, host_batch=False)
    assert dev.reads is None and dev.n == 4000
    dev.run()
    dev.run_cigars()
    dev.run_bam(None, sorted_output=True)
    dev.run_bgzf()
    dev.run_bai(77)
    _same(dev.bai(), snapgpu.bai_build(dev.bam(), dev.bgzf(), 3, 77))


@pytest.mark.parametrize("name", sorted(fabricated()))
def test_batch_form_on_the_fabricated_streams(world, name):
    raw, n_ref = fabricated()[name]
    for off in (0, 99):
        z, bai = world["aligner"].bai_build(raw, n_ref, off)
        _same(z, snapgpu.bgzf_compress_model(raw, eof=False), name)
        _same(bai, snapgpu.bai_build(raw, z, n_ref, off), name)


@pytest.mark.parametrize("n", SLICES)
def test_batch_form_on_slices(world, n):
    raw = _sorted_records(world, n, start=17)
    assert len(split(raw)) == n
    z, bai = world["aligner"].bai_build(raw, 3)
    _same(bai, snapgpu.bai_build(raw, z, 3), f"{n} reads")
    if n == 0:
        assert z == b"" and bai == b"BAI\1" + bytes([3, 0, 0, 0]) + bytes(3 * 8 + 8)


def test_buffer_reuse_growing_then_shrinking(world):
    al = world["aligner"]
    for start, n in ((0, 5), (7, 300), (0, 4000), (3999, 1), (0, 0), (1234, 33)):
        if n == 0:                                 # no records: the batch form, on the same aligner
            z, bai = al.bai_build(b"", 3, 5)
            raw = b""
        else:
            reads = world["reads"].slice(start, n)
            dev = _aligned(al, reads)
            dev.run_bam(reads, ids=world["ids"][start:start + n], sorted_output=True)
            dev.run_bgzf()
            dev.run_bai(5)
            bai, raw, z = dev.bai(), dev.bam(), dev.bgzf()
        _same(bai, snapgpu.bai_build(raw, z, 3, 5), f"{n} reads from {start}")


def test_ordered_before_the_next_run(world):
    """run_bam; run_bgzf; run_bai; run; run_cigars; bai() three times on one resident batch: the index passes
    read the records and the member offsets on the stream that wrote them, whatever the lanes do meanwhile."""
    al, reads, ids = world["aligner"], world["reads"], world["ids"]
    dev = _aligned(al, reads)
    dev.run_bam(reads, ids=ids, sorted_output=True)
    dev.run_bgzf()
    want = snapgpu.bai_build(dev.bam(), dev.bgzf(), 3, 40)
    for _ in range(3):
        dev.run_bam(reads, ids=ids, sorted_output=True)
        dev.run_bgzf()
        dev.run_bai(40)
        dev.run()
        dev.run_cigars()
        _same(dev.bai(), want)


def test_errors_leave_the_aligner_usable(world):
    al, reads, ids = world["aligner"], world["reads"].slice(0, 300), world["ids"][:300]
    dev = _aligned(al, reads)
    with pytest.raises(snapgpu.SnapGpuError, match="bam_resident_sorted"):
        dev.run_bai()                              # no BAM call at all
    dev.run_bam(reads, ids=ids)
    dev.run_bgzf()
    with pytest.raises(snapgpu.SnapGpuError, match="bam_resident_sorted"):
        dev.run_bai()                              # the last BAM call was not the sorted one
    dev.run_bam(reads, ids=ids, sorted_output=True)
    with pytest.raises(snapgpu.SnapGpuError, match="bam_bgzf_resident"):
        dev.run_bai()                              # no members of these records
    dev.run_bgzf()
    with pytest.raises(snapgpu.SnapGpuError, match="streamOffset"):
        dev.run_bai(1 << 48)
    dev.run_bai()
    dev.run_bam(reads, ids=ids, sorted_output=True)
    with pytest.raises(snapgpu.SnapGpuError, match="bam_bai_resident"):
        dev.bai()                                  # stale: the records were written again
    dev.run_bgzf()
    dev.run_bai()
    dev.run_bgzf()
    with pytest.raises(snapgpu.SnapGpuError, match="bam_bai_resident"):
        dev.bai()                                  # stale: the members were written again
    with pytest.raises(snapgpu.SnapGpuError, match="record 1: truncated"):
        raw = fabricated()["equal_pos"][0]
        al.bai_build(raw[:len(split(raw)[0]) + 10], 3)
    dev.run_bai(3)
    _same(dev.bai(), snapgpu.bai_build(dev.bam(), dev.bgzf(), 3, 3))


def test_write_sorted_bam(world, tmp_path):
    dev, reads, idx = world["dev"], world["reads"], world["idx"]
    dev.run_bam(reads, ids=world["ids"], sorted_output=True)
    path = str(tmp_path / "out.bam")
    text = snapgpu.sam_header(idx, "snap test", "test", sorted_output=True)
    snapgpu.write_sorted_bam(path, idx, text, dev)
    file_bytes, bai = open(path, "rb").read(), open(path + ".bai", "rb").read()
    head = snapgpu.bam_header(idx, text)
    whole = gzip.decompress(file_bytes)
    assert whole[:len(head)] == head and file_bytes[-28:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    raw = whole[len(head):]
    assert raw == dev.bam() and parse_bai(bai)["no_coor"] == sum(rec_fields(r)["ref"] < 0 for r in split(raw))
    rng = np.random.default_rng(5)
    recs = [rec_fields(r) for r in split(raw)]
    found = 0
    for ref in range(3):
        top = max(f["end"] for f in recs if f["ref"] == ref)
        regions = [(0, top)] + [(b, b + int(rng.choice([1, 50, 2000, 40000]))) for b in map(int, rng.integers(0, top, 20))]
        for k, (beg, end) in enumerate(regions):
            want = brute_force(raw, ref, beg, end)
            assert query(file_bytes, bai, ref, beg, end) == want, (ref, beg, end)
            found += len(want) if k == 0 else 0
    with_ref = sum(f["ref"] >= 0 for f in recs)
    assert found == with_ref, f"{found} of {with_ref} records with a refID came back from the whole-reference queries"
