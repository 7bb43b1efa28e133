"""Duplicate marking on the GPU (csrc/dupmark.hip: fields and scores, run numbering, best per group, mark,
check): byte-identical to the host model (snapgpu.bam_mark_duplicates), which test_dupmark_model.py holds
to the rule's restatement and to the reference's own marks.  Every expected value here comes from the model."""
import gzip
import random

import pytest

import snapgpu
from bai_cases import split
from dupmark_cases import fabricated, refusals

pytestmark = pytest.mark.gpu

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _same(got, want, what=""):
    if got != want:
        first = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
        pytest.fail(f"{what}: {len(got)} vs {len(want)} bytes, first difference at byte {first}")


def _aligned(al, reads):
    dev = al.upload(reads)
    dev.run()
    dev.run_cigars()
    return dev


@pytest.fixture(scope="module")
def world(gpu_available, small_world):
    """One aligner; reads 0-299 of small_world, read i in 1 + i % 4 copies with qualities and ids of their
    own, aligned once; never modified."""
    idx, reads = small_world["index"], small_world["reads"]
    rng = random.Random(400)
    copies, ids = [], []
    for i in range(300):
        bases = reads.get(i)[0]
        for c in range(1 + i % 4):
            copies.append((bases, bytes(33 + rng.randrange(20, 41) for _ in bases)))
            ids.append(b"read_%d_copy_%d" % (i, c))
    dup_reads = snapgpu.Reads.from_list(copies)
    al = snapgpu.BaseAligner(idx)
    return dict(idx=idx, reads=reads, aligner=al, dup_reads=dup_reads, dup_ids=ids, copies=copies,
                dev=_aligned(al, dup_reads), all_ids=[b"read_%d" % i for i in range(reads.n)])


@pytest.mark.parametrize("name", sorted(fabricated()))
def test_batch_form_on_the_fabricated_streams(world, name):
    raw, n_ref = fabricated()[name]
    want = snapgpu.bam_mark_duplicates(raw, n_ref)
    got = world["aligner"].bam_mark_duplicates(raw, n_ref)
    _same(got[0], want[0], name)
    assert got[1:] == want[1:], name
    again = world["aligner"].bam_mark_duplicates(got[0], n_ref)
    assert again == want, name
    k, d = world["aligner"].dupmark_ms()
    assert k > 0 and d >= 0


@pytest.mark.parametrize("name", sorted(refusals()))
def test_batch_form_refuses_and_leaves_the_buffer(world, name):
    import ctypes as C
    raw, n_ref, _ = refusals()[name]
    buf = C.create_string_buffer(raw, len(raw))
    marked, groups = C.c_uint64(7), C.c_uint64(7)
    rc = snapgpu.lib().snapgpu_bam_mark_duplicates_gpu(world["aligner"]._h, buf, len(raw), n_ref, C.byref(marked), C.byref(groups))
    assert rc < 0 and buf.raw == raw and (marked.value, groups.value) == (0, 0), name
    with pytest.raises(snapgpu.SnapGpuError):
        world["aligner"].bam_mark_duplicates(raw, n_ref)
    good, n = fabricated()["stray_marks"]                   # the aligner goes on
    assert world["aligner"].bam_mark_duplicates(good, n) == snapgpu.bam_mark_duplicates(good, n)


def _chain(dev, kept):
    """run_dupmark, run_bgzf, run_bai(77) on a batch whose sorted records are `kept`, all against the model."""
    want, n_marked, n_groups = snapgpu.bam_mark_duplicates(kept, 3)
    dev.run_dupmark()
    _same(dev.bam(), want, "marked records")
    assert dev.dupmark_stats() == (n_marked, n_groups)
    dev.run_bgzf()
    dev.run_bai(77)
    z = dev.bgzf()
    _same(gzip.decompress(z), want, "inflated members")
    _same(dev.bai(), snapgpu.bai_build(want, z, 3, 77), "index")
    return want, n_marked, n_groups


def test_resident_chain(world):
    dev = world["dev"]
    dev.run_bam(world["dup_reads"], ids=world["dup_ids"], sorted_output=True)
    kept = dev.bam()
    assert len(split(kept)) == 750
    want, n_marked, n_groups = _chain(dev, kept)
    assert n_marked >= 300 and n_groups >= 100 and want != kept
    k, d = world["aligner"].dupmark_ms()
    assert k > 0 and d == 0


def test_resident_chain_without_a_host_batch(world, tmp_path):
    path = tmp_path / "copies.fq"
    with open(path, "wb") as f:
        for name, (bases, quals) in zip(world["dup_ids"], world["copies"]):
            f.write(b"@" + name + b"\n" + bases + b"\n+\n" + quals + b"\n")
    dev = world["aligner"].upload_fastq(path, host_batch=False)
    assert dev.reads is None and dev.n == 750
    dev.run()
    dev.run_cigars()
    dev.run_bam(None, sorted_output=True)
    _, n_marked, _ = _chain(dev, dev.bam())
    assert n_marked >= 300


def test_states(world):
    al, reads, ids = world["aligner"], world["dup_reads"], world["dup_ids"]
    dev = _aligned(al, reads)
    with pytest.raises(snapgpu.SnapGpuError, match="bam_resident_sorted"):
        dev.run_dupmark()                          # no BAM call at all
    with pytest.raises(snapgpu.SnapGpuError, match="bam_dupmark_resident"):
        dev.dupmark_stats()
    dev.run_bam(reads, ids=ids)
    with pytest.raises(snapgpu.SnapGpuError, match="bam_resident_sorted"):
        dev.run_dupmark()                          # the last BAM call was not the sorted one
    dev.run_bam(reads, ids=ids, sorted_output=True)
    kept = dev.bam()
    with pytest.raises(snapgpu.SnapGpuError, match="bam_dupmark_resident"):
        dev.dupmark_stats()                        # no mark call since the BAM call
    dev.run_bgzf()
    dev.run_bai()
    assert gzip.decompress(dev.bgzf()) == kept
    dev.run_dupmark()
    with pytest.raises(snapgpu.SnapGpuError, match="bam_bgzf_resident"):
        dev.bgzf()                                 # stale: the records changed under the members
    with pytest.raises(snapgpu.SnapGpuError, match="bam_bai_resident"):
        dev.bai()
    with pytest.raises(snapgpu.SnapGpuError, match="bam_bgzf_resident"):
        dev.run_bai()                              # no members of the marked records yet
    want = snapgpu.bam_mark_duplicates(kept, 3)
    _same(dev.bam(), want[0], "marked")
    dev.run_dupmark()                              # twice: the same bytes
    _same(dev.bam(), want[0], "marked twice")
    assert dev.dupmark_stats() == want[1:]
    dev.run_bgzf()
    dev.run_bai()
    z = dev.bgzf()
    assert gzip.decompress(z) == want[0] and dev.bai() == snapgpu.bai_build(want[0], z, 3)
    dev.run_bam(reads, ids=ids, sorted_output=True)
    _same(dev.bam(), kept, "a fresh run_bam")      # unmarked again
    with pytest.raises(snapgpu.SnapGpuError, match="bam_dupmark_resident"):
        dev.dupmark_stats()


def test_buffer_reuse_growing_then_shrinking(world):
    al = world["aligner"]
    for start, n in ((0, 5), (7, 300), (0, 4000), (3999, 1), (0, 0), (1234, 33)):
        if n == 0:                                 # no records: the batch form, on the same aligner
            assert al.bam_mark_duplicates(b"", 3) == (b"", 0, 0)
            continue
        reads = world["reads"].slice(start, n)
        dev = _aligned(al, reads)
        dev.run_bam(reads, ids=world["all_ids"][start:start + n], sorted_output=True)
        want = snapgpu.bam_mark_duplicates(dev.bam(), 3)
        dev.run_dupmark()
        _same(dev.bam(), want[0], f"{n} reads from {start}")
        assert dev.dupmark_stats() == want[1:]


def test_write_sorted_bam(world, tmp_path):
    dev, reads, ids, idx = world["dev"], world["dup_reads"], world["dup_ids"], world["idx"]
    text = snapgpu.sam_header(idx, "snap test", "test", sorted_output=True)
    head = snapgpu.bam_header(idx, text)
    head_z = snapgpu.bgzf_compress(head, eof=False)
    dev.run_bam(reads, ids=ids, sorted_output=True)
    kept = dev.bam()
    dev.run_bgzf()
    plain_members = dev.bgzf()
    plain = str(tmp_path / "plain.bam")
    snapgpu.write_sorted_bam(plain, idx, text, dev)                           # the default: nothing marked
    assert open(plain, "rb").read() == head_z + plain_members and gzip.decompress(plain_members) == kept
    assert open(plain + ".bai", "rb").read() == snapgpu.bai_build(kept, plain_members, 3, len(head_z))
    dev.run_bam(reads, ids=ids, sorted_output=True)
    marked = str(tmp_path / "marked.bam")
    snapgpu.write_sorted_bam(marked, idx, text, dev, mark_duplicates=True)
    file_bytes = open(marked, "rb").read()
    want, n_marked, _ = snapgpu.bam_mark_duplicates(kept, 3)
    assert n_marked >= 300 and file_bytes[-28:] == EOF_BLOCK and file_bytes[:len(head_z)] == head_z
    _same(gzip.decompress(file_bytes), head + want, "the file's bytes")
    assert open(marked + ".bai", "rb").read() == snapgpu.bai_build(want, file_bytes[len(head_z):], 3, len(head_z))
