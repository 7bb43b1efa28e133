"""The device BGZF inflater (csrc/inflate.hip behind snapgpu_bgzf_inflate_gpu / BaseAligner.bgzf_inflate
and upload_fastq(bgzf=True)).  Expected bytes come from Python's gzip (inflate_cases.py), expected
refusals from the host model of the same decoder, expected batches from the plain-text device parser."""
import ctypes as C
import gzip

import numpy as np
import pytest

import snapgpu
from bgzf_cases import BLOCK, EOF_BLOCK, SIZED, SIZES, special
from fastq_cases import CASES, assert_same_fields, batch_fields, tile_cases
from inflate_cases import (BAD, CONTAINERS, EFORMAT, GOOD, bad_containers, bad_members, bgzf, deflate_of, fastq_text, good,
                           member, placed, refusal)

pytestmark = pytest.mark.gpu

TILE = tile_cases(snapgpu.FASTQ_TILE_BYTES)


def same_resident(got, want, what):
    """Two DeviceReads hold the same batch: what snapgpu_reads_upload defines of it (as test_fastq_gpu.py)."""
    g, w = got.peek(), want.peek()
    for k in ("n", "bytes", "maxLen", "extentHash"):
        assert g[k] == w[k], f"{what}: {k} {g[k]} != {w[k]}"
    for k in ("offsets", "lengths"):
        assert np.array_equal(g[k], w[k]), f"{what}: device {k} differ"
    for k in ("bases", "quals"):
        assert g[k] == w[k], f"{what}: device {k} differ on [0, bytes + 64)"
        assert g[k][w["bytes"]:] == bytes(64), f"{what}: device {k} slack is not zero"


@pytest.fixture(scope="module")
def world(gpu_available, small_world):
    al = snapgpu.BaseAligner(small_world["index"])
    for ms in (al.bgzf_inflate_ms, al.fastq_last_ms):
        with pytest.raises(snapgpu.SnapGpuError):
            ms()                    # no device inflate / parse on this aligner yet
    return {"al": al, "reads": small_world["reads"]}


@pytest.mark.parametrize("name", GOOD)
def test_good_streams(world, name):
    al = world["al"]
    stream, data = good()[name]
    got = al.bgzf_inflate(stream)
    assert got == data == (gzip.decompress(stream) if stream else b"")
    assert got == snapgpu.bgzf_inflate_model(stream)
    assert all(t >= 0 for t in al.bgzf_inflate_ms())


@pytest.mark.parametrize("name", BAD)
def test_bad_members_are_refused_as_the_model_refuses_them(world, name):
    al = world["al"]
    bad, status = bad_members()[name]
    for stream in (bad, placed(bad, [2]), placed(bad, [3, 1])):
        want = refusal(snapgpu.bgzf_inflate_model, stream)
        assert want[0] == EFORMAT and want[2] == status
        assert refusal(al.bgzf_inflate, stream) == want
    assert al.bgzf_inflate(good()["overlap"][0]) == good()["overlap"][1]      # and goes on working


@pytest.mark.parametrize("name", CONTAINERS)
def test_bad_containers(world, name):
    al = world["al"]
    stream = bad_containers()[name]
    assert refusal(al.bgzf_inflate, stream)[:2] == (EFORMAT, 1)
    used = C.c_uint64(7)                                     # the device entry's own walk
    assert snapgpu.lib().snapgpu_bgzf_inflate_gpu(al._h, stream, len(stream), None, 0, C.byref(used)) == EFORMAT
    assert used.value == 0 and "bgzf_inflate_gpu: member 1 at byte" in snapgpu.last_error()
    assert refusal(snapgpu.bgzf_inflate_model, stream)[:2] == (EFORMAT, 1)


@pytest.mark.parametrize("content", sorted(SIZED))
def test_round_trip_on_the_device(world, content):
    al = world["al"]
    for n in SIZES:
        data = SIZED[content](n)
        assert al.bgzf_inflate(al.bgzf_compress(data)) == data, n


def test_round_trip_of_the_special_contents(world):
    al = world["al"]
    for name, data in special().items():
        assert al.bgzf_inflate(al.bgzf_compress(data, eof=False)) == data, name


def test_stride(world):
    """More members than twice the kernel's waves, 1 - 200 bytes each with empty ones between: every wave
    goes round its loop more than twice, and the outputs start at every alignment."""
    al = world["al"]
    waves = al.bgzf_inflate_waves()
    assert waves > 0
    n = max(5000, 2 * waves + 3)
    rng = np.random.default_rng(77)
    sizes = rng.integers(1, 201, size=n)
    text = fastq_text()
    parts, stream = [], []
    for k in range(n):
        if k % 5 == 2:
            stream.append(EOF_BLOCK)
            continue
        at = int(rng.integers(0, len(text) - 200))
        piece = text[at:at + int(sizes[k])]
        parts.append(piece)
        stream.append(member(deflate_of(piece, level=int(k % 10)), piece))
    stream, data = b"".join(stream), b"".join(parts)
    assert snapgpu.bgzf_inflate_size(stream) == (len(data), n) and 200_000 < len(data) < 1_000_000
    assert al.bgzf_inflate(stream) == data
    u, k, d = al.bgzf_inflate_ms()
    assert u >= 0 and k >= 0 and d >= 0


def _check_parser(al, text, what, tmp_path):
    """upload_fastq(bgzf(text), bgzf=True) against upload_fastq(text): resident arrays, host batch, no host batch."""
    path = tmp_path / "case.fq.gz"
    for clipping in (0, 3):
        plain = al.upload_fastq(text, clipping=clipping, name="case")
        want = batch_fields(plain.reads)
        for block in (1000, BLOCK):
            stream = bgzf(text, block=block) + (EOF_BLOCK if block == 1000 else b"")
            path.write_bytes(stream)
            for source in (stream, path):
                tag = f"{what}, clipping {clipping}, block {block}, {'file' if source is path else 'bytes'}"
                dev = al.upload_fastq(source, clipping=clipping, name="case", bgzf=True)
                assert dev.n == plain.n
                assert_same_fields(batch_fields(dev.reads), want, tag)
                same_resident(dev, plain, tag)
                bare = al.upload_fastq(source, clipping=clipping, host_batch=False, bgzf=True)
                assert bare.reads is None
                same_resident(bare, plain, tag + ", no host batch")
    u, k, d = al.fastq_last_ms()
    assert u >= 0 and k >= 0 and d >= 0 and k >= al.bgzf_inflate_ms()[1] >= 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_parser_equality_on_the_nasty_cases(world, name, tmp_path):
    _check_parser(world["al"], CASES[name], name, tmp_path)      # "empty" and "no_final_newline" are among them


@pytest.mark.parametrize("name", sorted(TILE))
def test_parser_equality_on_the_tile_edges(world, name, tmp_path):
    _check_parser(world["al"], TILE[name], name, tmp_path)


def test_parser_equality_on_the_golden_reads(world, tmp_path):
    _check_parser(world["al"], fastq_text(), "single_reads.fq", tmp_path)


def test_empty_streams_are_empty_batches(world):
    al = world["al"]
    for stream in (b"", EOF_BLOCK, EOF_BLOCK * 3):
        dev = al.upload_fastq(stream, bgzf=True)
        assert dev.n == 0 and dev.reads.n == 0
        assert al.upload_fastq(stream, bgzf=True, host_batch=False).reads is None


def test_a_bad_member_inside_a_fastq_stream(world, tmp_path):
    al = world["al"]
    text = fastq_text()[:30000]
    stream = bgzf(text, block=5000)
    first = len(bgzf(text[:5000]))
    for name in ("crc", "truncated", "dist_before_start"):
        bad = stream[:first] + bad_members()[name][0] + stream[first:]
        want = refusal(snapgpu.bgzf_inflate_model, bad)
        for source in (bad, tmp_path / "bad.fq.gz"):
            if source is not bad:
                source.write_bytes(bad)
            got = refusal(lambda s: al.upload_fastq(s, clipping=3, bgzf=True), source)
            assert got == (EFORMAT, 1, want[2])
        good_dev = al.upload_fastq(stream, clipping=3, bgzf=True)        # the aligner runs the next call
        same_resident(good_dev, al.upload_fastq(text, clipping=3), f"after {name}")
    for name in ("flg0", "trailing"):
        assert refusal(lambda s: al.upload_fastq(s, bgzf=True), bad_containers()[name])[:2] == (EFORMAT, 1)
    with pytest.raises(snapgpu.SnapGpuError) as e:
        al.upload_fastq(tmp_path / "missing.fq.gz", bgzf=True)
    assert "cannot open" in str(e.value)


def test_end_to_end(world, tmp_path):
    """small_world's reads as FASTQ: the BGZF stream through upload_fastq -> run -> run_cigars -> run_sam
    gives the SAM text of the plain-text chain."""
    al = world["al"]
    path = tmp_path / "reads.fq"
    world["reads"].write_fastq(path)
    text = path.read_bytes()
    sams = []
    for dev in (al.upload_fastq(text, clipping=3), al.upload_fastq(bgzf(text), clipping=3, bgzf=True)):
        assert dev.n == 4000
        dev.run()
        dev.run_cigars()
        dev.run_sam(dev.reads)
        sams.append(dev.sam())
    assert sams[0] == sams[1] and sams[0].count(b"\n") == 4000
    u, k, d = al.fastq_last_ms()
    assert u >= 0 and k >= 0 and d >= 0
