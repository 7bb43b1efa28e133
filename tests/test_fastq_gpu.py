"""The device FASTQ parser (csrc/fastq_parse.hip behind snapgpu_fastq_upload / BaseAligner.upload_fastq).
Every expected value is the host parser's batch, clipped by snapgpu_reads_clip, and what
snapgpu_reads_upload makes of it; the host parser itself is pinned in test_fastq_buffer.py."""
import ctypes as C

import numpy as np
import pytest

import snapgpu
from snapgpu import _ffi
from fastq_cases import (BAD, BAD_MESSAGE, CASES, assert_same_fields, batch_fields, host_batch, random_text, tile_cases)

pytestmark = pytest.mark.gpu

T = snapgpu.FASTQ_TILE_BYTES
TILE = tile_cases(T)
EINVAL, ENOMEM, EFORMAT = -1, -3, -5   # include/snapgpu.h


@pytest.fixture(scope="module")
def world(gpu_available, small_world):
    al = snapgpu.BaseAligner(small_world["index"])
    with pytest.raises(snapgpu.SnapGpuError):
        al.fastq_last_ms()          # no device parse on this aligner yet
    return {"al": al, "reads": small_world["reads"]}


def same_resident(got, want, what):
    """Two DeviceReads hold the same batch: what snapgpu_reads_upload defines of it."""
    g, w = got.peek(), want.peek()
    for k in ("n", "bytes", "maxLen", "extentHash"):
        assert g[k] == w[k], f"{what}: {k} {g[k]} != {w[k]}"
    for k in ("offsets", "lengths"):
        assert np.array_equal(g[k], w[k]), f"{what}: device {k} differ"
    for k in ("bases", "quals"):
        assert g[k] == w[k], f"{what}: device {k} differ on [0, bytes + 64)"
        assert g[k][w["bytes"]:] == bytes(64), f"{what}: device {k} slack is not zero"


def check_text(al, text, what, source=None, clippings=(0, 1, 2, 3)):
    """upload_fastq(source or text) against the host parser + clip + upload, host batch and device arrays."""
    for clipping in clippings:
        want = host_batch(text, clipping)
        ref = al.upload(want)                      # nUploads becomes 1, as the device parser reports it
        dev = al.upload_fastq(text if source is None else source, clipping=clipping, name="case")
        assert dev.n == want.n
        assert_same_fields(batch_fields(dev.reads), batch_fields(want), f"{what}, clipping {clipping}")
        same_resident(dev, ref, f"{what}, clipping {clipping}")
        bare = al.upload_fastq(text if source is None else source, clipping=clipping, host_batch=False)
        assert bare.reads is None
        same_resident(bare, ref, f"{what}, clipping {clipping}, no host batch")
    u, k, d = al.fastq_last_ms()
    assert u >= 0 and k >= 0 and d >= 0


def test_constants():
    assert snapgpu.lib().snapgpu_fastq_tile_bytes() == T
    assert snapgpu.FASTQ_HOST_BATCH == 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_nasty_cases(world, name):
    check_text(world["al"], CASES[name], name)


@pytest.mark.parametrize("name", sorted(TILE))
def test_tile_edges(world, name):
    text = TILE[name]
    check_text(world["al"], text, name)
    if name.startswith("long_line"):
        dev = world["al"].upload_fastq(text, clipping=0)
        assert dev.peek(arrays=False)["maxLen"] == T + 5000 > 1024


def test_file_form(world, tmp_path):
    for name in ("four_plus_2", "no_final_newline", "empty"):
        p = tmp_path / f"{name}.fq"
        p.write_bytes(CASES[name])
        check_text(world["al"], CASES[name], f"file {name}", source=p, clippings=(0, 3))
    p = tmp_path / "tile.fq"
    p.write_bytes(TILE["record_straddles_2T+1"])
    check_text(world["al"], TILE["record_straddles_2T+1"], "file tile", source=p, clippings=(3,))
    with pytest.raises(snapgpu.SnapGpuError) as e:
        world["al"].upload_fastq(tmp_path / "missing.fq")
    assert "cannot open" in str(e.value)


def _raw_upload(al, text, n_bytes, name, clipping, flags):
    d, r = C.c_void_p(7), C.pointer(_ffi.Reads())
    buf = C.create_string_buffer(text, len(text) + 1)
    rc = snapgpu.lib().snapgpu_fastq_upload(al._h, buf, n_bytes, name, clipping, flags, C.byref(d), C.byref(r))
    return rc, d, r


@pytest.mark.parametrize("name", sorted(BAD))
def test_malformed_headers(world, name, tmp_path):
    al = world["al"]
    rc, d, r = _raw_upload(al, BAD[name], len(BAD[name]), b"some name", 3, 1)
    assert rc == EFORMAT and not d.value and not r
    assert snapgpu.last_error() == BAD_MESSAGE + "some name"
    with pytest.raises(snapgpu.SnapGpuError) as e:
        snapgpu.Reads.from_fastq_bytes(BAD[name], name="some name")
    assert snapgpu.last_error() in str(e.value)              # the host parser's message
    p = tmp_path / "bad.fq"
    p.write_bytes(BAD[name])
    with pytest.raises(snapgpu.SnapGpuError) as e:
        al.upload_fastq(p, clipping=0, host_batch=False)
    assert f"({EFORMAT})" in str(e.value) and (BAD_MESSAGE + str(p)) in str(e.value)
    check_text(al, CASES["crlf"], "after a refused text", clippings=(3,))


def test_bad_arguments(world):
    al = world["al"]
    text = CASES["crlf"]
    for clipping in (-1, 4):
        rc, d, r = _raw_upload(al, text, len(text), b"x", clipping, 1)
        assert rc == EINVAL and not d.value and not r
    assert _raw_upload(al, text, len(text), None, 0, 1)[0] == EINVAL          # no name
    assert _raw_upload(al, text, len(text), b"x", 0, 2)[0] == EINVAL          # an unknown flag
    fn = snapgpu.lib().snapgpu_fastq_upload
    d = C.c_void_p()
    assert fn(al._h, None, 5, b"x", 0, 0, C.byref(d), None) == EINVAL         # no text
    assert fn(al._h, text, len(text), b"x", 0, 1, C.byref(d), None) == EINVAL # host batch asked for, nowhere to put it
    assert fn(al._h, text, len(text), b"x", 0, 0, None, None) == EINVAL
    assert fn(None, text, len(text), b"x", 0, 0, C.byref(d), None) == EINVAL
    assert fn(al._h, text, len(text), b"x", 0, 0, C.byref(d), None) == 0 and d.value   # readsOut may be NULL without the flag
    snapgpu.lib().snapgpu_device_reads_free(d)


def test_memory_ceiling(world):
    """A text larger than the device's free memory is refused before anything is allocated or read:
    the claimed size is checked against hipMemGetInfo first, so the 16 bytes behind it are never touched."""
    al = world["al"]
    rc, d, r = _raw_upload(al, b"@a\nACGT\n+\nIIII\n", 1 << 46, b"huge", 0, 1)
    assert rc == ENOMEM and not d.value and not r
    msg = snapgpu.last_error()
    assert "needs" in msg and "are free" in msg
    check_text(al, CASES["clip_leaves_50"], "after a refused size", clippings=(3,))


def test_clip_edges_on_the_device(world):
    """The clip cases again, by value: what the device leaves in dOffsets / dLengths."""
    al = world["al"]
    for name, want in {"clip_all_hash": [(0, 60)], "clip_leaves_49": [(0, 60), (60, 60), (120, 60)],
                       "clip_leaves_50": [(5, 50), (70, 50), (120, 50)], "clip_front_only": [(7, 53)],
                       "clip_back_only": [(0, 52)]}.items():
        p = al.upload_fastq(CASES[name], clipping=3, host_batch=False).peek()
        assert list(zip(p["offsets"].tolist(), p["lengths"].tolist())) == want, name


def test_random_records(world):
    al = world["al"]
    text = random_text(2024, 5000)
    check_text(al, text, "random")
    a, b = al.upload_fastq(text, clipping=3), al.upload_fastq(text, clipping=3)
    assert_same_fields(batch_fields(a.reads), batch_fields(b.reads), "the same text twice")
    same_resident(a, b, "the same text twice")


@pytest.fixture(scope="module")
def chain(world, tmp_path_factory):
    """small_world's 4,000 reads as a FASTQ file, every seventh (and the last) with '#' runs at both ends,
    through the host chain once: parse, clip at 3, upload, run, CIGARs, SAM, BAM, BGZF."""
    al = world["al"]
    path = tmp_path_factory.mktemp("fastq_gpu") / "reads.fq"
    world["reads"].write_fastq(path)
    lines = path.read_bytes().split(b"\n")
    for r in list(range(0, 4000, 7)) + [3999]:
        q = lines[4 * r + 3]
        lines[4 * r + 3] = b"#" * 5 + q[5:-8] + b"#" * 8
    path.write_bytes(b"\n".join(lines))
    reads = snapgpu.Reads.from_fastq(path)
    front, _ = reads.clip(3)
    assert (front == 5).sum() >= 572
    dev = al.upload(reads)
    dev.run()
    out = {"path": path, "results": dev.results().copy()}
    dev.run_cigars()
    dev.run_sam(reads)
    out["sam"] = dev.sam()
    dev.run_bam(reads)
    out["bam"] = dev.bam()
    dev.run_bgzf()
    out["bgzf"] = dev.bgzf()
    return out


def test_chain_from_the_device_parser(world, chain):
    al = world["al"]
    dev = al.upload_fastq(chain["path"], clipping=3)
    assert dev.n == 4000 and dev.reads.n == 4000
    dev.run()
    got = dev.results()
    assert got.tobytes() == chain["results"].tobytes()      # all 64 bytes of every record
    assert (got["result"] == snapgpu.SingleHit).sum() > 3000
    dev.run_cigars()
    dev.run_sam(dev.reads)                                  # the pair passes the resident extent check
    assert dev.sam() == chain["sam"] and chain["sam"].count(b"\n") == 4000
    dev.run_bam(dev.reads)
    assert dev.bam() == chain["bam"]
    dev.run_bgzf()
    assert dev.bgzf() == chain["bgzf"]


def test_chain_without_host_batch(world, chain):
    dev = world["al"].upload_fastq(chain["path"], clipping=3, host_batch=False)
    assert dev.reads is None and dev.n == 4000
    dev.run()
    assert dev.results().tobytes() == chain["results"].tobytes()
