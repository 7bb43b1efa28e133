"""The host model of the device BGZF compressor (snapgpu.bgzf_compress_model: csrc/host/bgzf.cpp, the
serial restatement of csrc/bgzf_block.h): needs no GPU.  Its members are not zlib's, so the expected
values are the format's own rules and what Python's zlib / gzip inflate from them."""
import ctypes as C
import hashlib
import heapq
import os
import subprocess
import sys

import numpy as np
import pytest

import snapgpu
from bgzf_cases import BLOCK, EOF_BLOCK, SIZED, SIZES, btype, check_stream, members, special

EINVAL = -1   # SNAPGPU_EINVAL (include/snapgpu.h)
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("content", sorted(SIZED))
def test_round_trip_and_structure(content, n):
    data = SIZED[content](n)
    out = snapgpu.bgzf_compress_model(data)
    mem = check_stream(out, data, eof=True)
    assert snapgpu.bgzf_compress_model(data, eof=False) + EOF_BLOCK == out
    if content == "random":                       # nothing to gain: every member is stored
        assert [btype(out, at) for at, _ in mem[:-1]] == [0] * (len(mem) - 1)
        assert [size for _, size in mem[:-1]] == [min(BLOCK, n - k * BLOCK) + 31 for k in range(len(mem) - 1)]
    else:                                         # a period: one match per 258 bytes, two bytes each at the most
        for k, (at, size) in enumerate(mem[:-1]):
            if min(BLOCK, n - k * BLOCK) >= BLOCK - 1:
                assert btype(out, at) == 2 and size < 2000


@pytest.mark.parametrize("name", ["one_byte_1", "one_byte_2", "all_256_once", "motif_32768", "motif_32769",
                                  "motif_across_blocks", "fibonacci", "rna_paired", "single"])
def test_special_contents(name):
    data = special()[name]
    out = snapgpu.bgzf_compress_model(data, eof=False)
    mem = check_stream(out, data, eof=False)
    if name.startswith("motif") or name == "fibonacci":
        assert all(btype(out, at) == 2 for at, _ in mem)
    if name == "motif_32768":
        # the motif's second copy is one match at the farthest distance; one byte farther it is literals
        far = snapgpu.bgzf_compress_model(special()["motif_32769"], eof=False)
        assert len(out) < len(far)


def _order0_bytes(data):
    """Sum over the blocks of the Huffman-coded size of the block's byte histogram, headers not counted:
    no encoder without matches gets under it."""
    bits = 0
    for k in range(0, len(data), BLOCK):
        counts = np.bincount(np.frombuffer(data[k:k + BLOCK], dtype=np.uint8), minlength=256)
        heap = [int(c) for c in counts if c]
        heapq.heapify(heap)
        if len(heap) == 1:
            bits += heap[0]
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            bits += a + b                          # every merge adds one bit to each symbol below it
            heapq.heappush(heap, a + b)
    return bits / 8


@pytest.mark.parametrize("name", ["rna_paired", "single"])
def test_it_compresses_the_golden_records(name):
    data = special()[name]
    out = snapgpu.bgzf_compress_model(data, eof=False)
    bound = _order0_bytes(data)
    print(f"{name}: {len(data)} bytes -> {len(out)}, order-0 bound {bound:.0f} ({len(out) / bound:.3f})")
    assert all(btype(out, at) == 2 for at, _ in members(out))
    assert len(out) < bound


def test_bytes_do_not_depend_on_the_thread_count():
    code = ("import sys, hashlib; sys.path.insert(0, %r); sys.path.insert(0, %r); import snapgpu\n"
            "from bgzf_cases import special\n"
            "print(snapgpu.host_threads(), *[hashlib.sha256(snapgpu.bgzf_compress_model(special()[k])).hexdigest()"
            " for k in ('rna_paired', 'single', 'motif_across_blocks')])"
            % (os.path.join(ROOT, "snap-rnaseq_amd"), HERE))
    outs = {}
    for threads in (1, 16):
        env = dict(os.environ, SNAPGPU_HOST_THREADS=str(threads))
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
        t, *digests = p.stdout.split()
        assert int(t) == threads
        outs[threads] = digests
    assert outs[1] == outs[16] and len(outs[1]) == 3
    assert outs[1][0] == hashlib.sha256(snapgpu.bgzf_compress_model(special()["rna_paired"])).hexdigest()


def test_a_whole_file():
    header = b"BAM\1" + (1234).to_bytes(4, "little") + b"@HD\tVN:1.4\n" * 100
    records = special()["single"]
    out = snapgpu.bgzf_compress(header, eof=False) + snapgpu.bgzf_compress_model(records)
    import gzip
    assert gzip.decompress(out) == header + records


def test_errors():
    fn = snapgpu.lib().snapgpu_bgzf_compress_model
    used = C.c_uint64(7)
    buf = C.create_string_buffer(64)
    assert fn(None, 5, 1, buf, 64, C.byref(used)) == EINVAL and "null argument" in snapgpu.last_error()
    assert fn(b"abcde", 5, 1, buf, 64, None) == EINVAL
    data = bytes(1000)
    need = len(snapgpu.bgzf_compress_model(data))
    assert fn(data, len(data), 1, buf, need - 1, C.byref(used)) != 0
    assert used.value == need and "too small" in snapgpu.last_error()
    assert fn(data, len(data), 1, None, 0, C.byref(used)) != 0 and used.value == need
    used.value = 0
    assert fn(None, 0, 0, None, 0, C.byref(used)) == 0 and used.value == 0      # nothing in, nothing out
    assert fn(None, 0, 1, buf, 64, C.byref(used)) == 0 and buf.raw[:28] == EOF_BLOCK and used.value == 28


def test_stand_alone_program_under_sanitizers(tmp_path):
    """tests/c/bgzf_model_test.cpp: the model's sources with -fsanitize=address,undefined in a program of
    their own, over the contents above and 3,000 seeded random inputs, inflated by zlib."""
    exe = tmp_path / "bgzf_model_test"
    src = os.path.join(ROOT, "snap-rnaseq_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", src, "-I", os.path.join(src, "host"),
                    os.path.join(HERE, "c", "bgzf_model_test.cpp"), os.path.join(src, "host", "bgzf.cpp"),
                    os.path.join(src, "host", "threads.cpp"), "-o", str(exe), "-lz", "-lpthread"],
                   check=True, capture_output=True)
    out = subprocess.run([str(exe), "3000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and ", 0 failed" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
