"""The host FASTQ parser over a buffer (snapgpu_reads_from_fastq_buffer) and the record rule it shares
with the device parser (csrc/fastq_record.h): needs no GPU.  The file form is pinned to the reference
reader by the golden fixtures; here the buffer form is pinned to the file form, and both, with
snapgpu_reads_clip, to a pure-Python restatement of the rule (fastq_cases.py)."""
import glob
import os
import subprocess

import pytest

import snapgpu
from fastq_cases import (BAD, BAD_MESSAGE, CASES, assert_same_fields, batch_fields, host_batch, py_batch, random_text,
                         tile_cases)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN_FQ = sorted(glob.glob(os.path.join(HERE, "golden", "*.fq")))
TILE = tile_cases(snapgpu.FASTQ_TILE_BYTES)


def test_there_are_golden_files():
    assert len(GOLDEN_FQ) >= 10


@pytest.mark.parametrize("path", GOLDEN_FQ, ids=os.path.basename)
def test_buffer_form_equals_file_form(path):
    data = open(path, "rb").read()
    want = batch_fields(snapgpu.Reads.from_fastq(path))
    assert want["n"] == data.count(b"\n") // 4 > 0
    assert_same_fields(batch_fields(snapgpu.Reads.from_fastq_bytes(data)), want, os.path.basename(path))
    assert_same_fields(want, py_batch(data, 0), "restatement")


@pytest.mark.parametrize("path", GOLDEN_FQ[:3], ids=os.path.basename)
def test_file_form_clipped_equals_the_restatement(path):
    reads = snapgpu.Reads.from_fastq(path)
    reads.clip(3)
    assert_same_fields(batch_fields(reads), py_batch(open(path, "rb").read(), 3), os.path.basename(path))


@pytest.mark.parametrize("clipping", [0, 1, 2, 3])
@pytest.mark.parametrize("name", sorted(CASES) + sorted(TILE))
def test_nasty_cases_against_the_restatement(name, clipping):
    text = CASES[name] if name in CASES else TILE[name]
    got = batch_fields(host_batch(text, clipping))
    assert got["nUploads"] == 0
    assert_same_fields(got, py_batch(text, clipping), name)


def test_the_cases_are_what_their_names_say():
    T = snapgpu.FASTQ_TILE_BYTES
    assert py_batch(CASES["empty"], 0)["n"] == 0 and py_batch(CASES["three_lines"], 0)["n"] == 0
    assert py_batch(CASES["no_final_newline"], 0)["n"] == 1
    assert [py_batch(CASES[f"four_plus_{k}"], 0)["n"] for k in (1, 2, 3)] == [4, 4, 4]
    assert py_batch(CASES["short_quals"], 0)["quals"][:12] == b"III\0\0\0\0\0\0\0\0\0"
    for k, (f, n) in {"clip_all_hash": (0, 60), "clip_front_only": (7, 53), "clip_back_only": (0, 52)}.items():
        b = py_batch(CASES[k], 3)
        assert (b["frontClipped"][0], b["lengths"][0]) == (f, n), k
    assert list(py_batch(CASES["clip_leaves_49"], 3)["lengths"]) == [60, 60, 60]
    assert list(py_batch(CASES["clip_leaves_50"], 3)["lengths"]) == [50, 50, 50]
    assert sorted({len(t) for k, t in TILE.items() if not k.startswith("long")}) == [T - 1, T, T + 1, 2 * T + 1]
    assert TILE["nl_last_of_tile_T+0"][T - 1:T] == b"\n" and TILE["nl_first_of_next_T+1"][T:T + 1] == b"\n"
    assert TILE["nl_last_of_tile_2T+1"][T - 1:T] == b"\n" and TILE["nl_first_of_next_2T+1"][T:T + 1] == b"\n"
    assert b"\n" not in TILE["record_straddles_2T+1"][T - 2:T + 2]
    long = py_batch(TILE["long_line"], 3)
    assert long["unclippedLength"][1] == T + 5000 and long["frontClipped"][1] == 3 and long["lengths"][1] == T + 5000 - 7


@pytest.mark.parametrize("name", sorted(BAD))
def test_records_without_header_are_refused(name):
    assert py_batch(BAD[name], 0) is None
    with pytest.raises(snapgpu.SnapGpuError) as e:
        snapgpu.Reads.from_fastq_bytes(BAD[name], name="some name")
    assert (BAD_MESSAGE + "some name") in str(e.value)


def test_file_form_names_the_path_in_its_error(tmp_path):
    p = tmp_path / "bad.fq"
    p.write_bytes(BAD["bad_last"])
    with pytest.raises(snapgpu.SnapGpuError) as e:
        snapgpu.Reads.from_fastq(p)
    assert (BAD_MESSAGE + str(p)) in str(e.value)


def test_random_records_against_the_restatement():
    text = random_text(11, 1500)
    for clipping in (0, 3):
        assert_same_fields(batch_fields(host_batch(text, clipping)), py_batch(text, clipping), f"random, clipping {clipping}")


def test_null_arguments():
    fn = snapgpu.lib().snapgpu_reads_from_fastq_buffer
    assert not fn(None, 5, b"x") and "null argument" in snapgpu.last_error()
    assert not fn(b"@a\nA\n+\nI\n", 9, None)
    empty = fn(None, 0, b"x")
    assert empty and empty.contents.n == 0
    snapgpu.lib().snapgpu_reads_free(empty)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """tests/c/fastq_record_test.cpp: fastq_record.h, the buffer parser and snapgpu_reads_clip, built with
    -fsanitize=address,undefined in a program of their own, over the texts above and 3,000 seeded random
    ones, against a byte-at-a-time parser inside the program."""
    exe = tmp_path / "fastq_record_test"
    src = os.path.join(ROOT, "snap-rnaseq_amd", "csrc")
    host = [os.path.join(src, "host", f) for f in ("reads.cpp", "sam.cpp", "threads.cpp", "genome.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", src, "-I", os.path.join(src, "host"),
                    os.path.join(HERE, "c", "fastq_record_test.cpp"), *host, "-o", str(exe), "-lpthread"],
                   check=True, capture_output=True)
    files = []
    for name, text in {**CASES, **BAD, **TILE}.items():
        files.append(tmp_path / f"{name}.fq")
        files[-1].write_bytes(text)
    out = subprocess.run([str(exe), "3000", *map(str, files)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and f"{3000 + len(files)} cases, 0 failed" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
