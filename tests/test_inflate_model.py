"""BGZF inflated on the host (csrc/host/inflate.cpp): snapgpu.bgzf_inflate (zlib on the host threads)
and snapgpu.bgzf_inflate_model (csrc/inflate_block.h, the decoder the device kernel compiles): needs
no GPU.  Expected bytes come from Python's zlib / gzip (inflate_cases.py)."""
import ctypes as C
import gzip
import hashlib
import os
import re
import subprocess
import sys

import pytest

import snapgpu
from bgzf_cases import BLOCK, EOF_BLOCK, SIZED, SIZES, special
from inflate_cases import (BAD, CONTAINERS, EFORMAT, EINVAL, GOOD, bad_containers, bad_members, bgzf, good, placed,
                           refusal)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BOTH = [snapgpu.bgzf_inflate, snapgpu.bgzf_inflate_model]


def test_the_case_lists_are_the_cases():
    assert sorted(GOOD) == sorted(good()) and sorted(BAD) == sorted(bad_members()) and sorted(CONTAINERS) == sorted(bad_containers())


@pytest.mark.parametrize("name", GOOD)
def test_good_streams(name):
    stream, data = good()[name]
    assert (gzip.decompress(stream) if stream else b"") == data
    for fn in BOTH:
        assert fn(stream) == data, fn.__name__
    size, members = snapgpu.bgzf_inflate_size(stream)
    assert size == len(data)
    if name == "empty_between":
        assert members == 6
    if name == "fq_block1000":
        assert members == 40


@pytest.mark.parametrize("name", BAD)
def test_bad_members_are_refused(name):
    bad, status = bad_members()[name]
    for fn in BOTH:
        assert refusal(fn, bad)[:2] == (EFORMAT, 0)
        assert refusal(fn, placed(bad, [2]))[:2] == (EFORMAT, 2)        # third among five
        assert refusal(fn, placed(bad, [3, 1]))[:2] == (EFORMAT, 1)     # two bad ones: the lower index
    assert refusal(snapgpu.bgzf_inflate_model, placed(bad, [2])) == (EFORMAT, 2, status)
    assert snapgpu.bgzf_inflate_size(placed(bad, [2]))[1] == 5            # the walk has nothing against it


def test_two_different_bad_members_report_the_lower():
    b = bad_members()
    stream = placed(b["crc"][0], [4], n=6)
    first = bgzf(b"member 0 " * 50)
    stream = stream[:len(first)] + b["btype3"][0] + stream[len(first):]   # now member 1 of 7, the CRC one member 5
    assert refusal(snapgpu.bgzf_inflate_model, stream) == (EFORMAT, 1, b["btype3"][1])
    assert refusal(snapgpu.bgzf_inflate, stream)[:2] == (EFORMAT, 1)


@pytest.mark.parametrize("name", CONTAINERS)
def test_bad_containers_are_refused_by_the_walk(name):
    stream = bad_containers()[name]
    at = len(bgzf(b"a good member"))
    for fn in BOTH + [snapgpu.bgzf_inflate_size]:
        with pytest.raises(snapgpu.SnapGpuError) as e:
            fn(stream)
        assert "(%d)" % EFORMAT in str(e.value) and "member 1 at byte %d" % at in str(e.value)
        if name in ("flg0", "no_bc"):
            assert "gzip, but not BGZF" in str(e.value)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("content", sorted(SIZED))
def test_the_model_inflates_the_compressor_model(content, n):
    data = SIZED[content](n)
    assert snapgpu.bgzf_inflate_model(snapgpu.bgzf_compress_model(data)) == data


@pytest.mark.parametrize("name", ["one_byte_1", "one_byte_2", "all_256_once", "motif_32768", "motif_32769",
                                  "motif_across_blocks", "fibonacci", "rna_paired", "single"])
def test_the_model_inflates_the_compressor_models_special_contents(name):
    data = special()[name]
    stream = snapgpu.bgzf_compress_model(data, eof=False)
    assert snapgpu.bgzf_inflate_model(stream) == data
    assert snapgpu.bgzf_inflate(stream) == data
    assert snapgpu.bgzf_inflate_size(stream) == (len(data), (len(data) + BLOCK - 1) // BLOCK)


def test_size_contract_and_null_arguments():
    stream, data = good()["fq_block1000"]
    used = C.c_uint64(7)
    buf = C.create_string_buffer(len(data))
    for fn in (snapgpu.lib().snapgpu_bgzf_inflate, snapgpu.lib().snapgpu_bgzf_inflate_model):
        assert fn(None, 5, buf, len(data), C.byref(used)) == EINVAL and "null argument" in snapgpu.last_error()
        assert fn(stream, len(stream), buf, len(data), None) == EINVAL
        used.value = 0
        assert fn(stream, len(stream), buf, len(data) - 1, C.byref(used)) == EINVAL
        assert used.value == len(data) and "too small" in snapgpu.last_error()
        assert fn(stream, len(stream), None, 0, C.byref(used)) == EINVAL and used.value == len(data)
        assert fn(stream, len(stream), buf, len(data), C.byref(used)) == 0 and buf.raw == data
        assert fn(None, 0, None, 0, C.byref(used)) == 0 and used.value == 0            # nothing in, nothing out
        assert fn(EOF_BLOCK, 28, None, 0, C.byref(used)) == 0 and used.value == 0
    size, members = C.c_uint64(), C.c_uint64()
    fn = snapgpu.lib().snapgpu_bgzf_inflate_size
    assert fn(None, 5, C.byref(size), C.byref(members)) == EINVAL
    assert fn(stream, len(stream), None, C.byref(members)) == EINVAL
    assert fn(stream, len(stream), C.byref(size), None) == EINVAL
    assert fn(stream, len(stream), C.byref(size), C.byref(members)) == 0 and (size.value, members.value) == (len(data), 40)


def test_bytes_do_not_depend_on_the_thread_count():
    code = ("import sys, hashlib; sys.path.insert(0, %r); sys.path.insert(0, %r); import snapgpu\n"
            "from inflate_cases import good, bad_members, placed\n"
            "out = [hashlib.sha256(f(good()[k][0])).hexdigest() for k in ('fq_level6', 'fq_block1000', 'empty_between')"
            " for f in (snapgpu.bgzf_inflate, snapgpu.bgzf_inflate_model)]\n"
            "try:\n    snapgpu.bgzf_inflate_model(placed(bad_members()['crc'][0], [7, 3, 5], n=9))\n"
            "except snapgpu.SnapGpuError as e:\n    out.append(str(e).split(': ', 1)[1].replace(' ', '_'))\n"
            "print(snapgpu.host_threads(), *out)"
            % (os.path.join(ROOT, "snap-rnaseq_amd"), HERE))
    outs = {}
    for threads in (1, 16):
        env = dict(os.environ, SNAPGPU_HOST_THREADS=str(threads))
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
        t, *rest = p.stdout.split()
        assert int(t) == threads
        outs[threads] = rest
    assert outs[1] == outs[16] and len(outs[1]) == 7
    assert outs[1][0] == outs[1][1] == hashlib.sha256(good()["fq_level6"][1]).hexdigest()
    assert "member_3_" in outs[1][6]


def test_stand_alone_program_under_sanitizers(tmp_path):
    """tests/c/inflate_model_test.cpp: the model's sources with -fsanitize=address,undefined in a program of
    their own, over 3,000 seeded random inputs compressed by zlib and by the compressor model, and their
    damaged versions, each held in a buffer of exactly its size: where the decoder's bounds are proven."""
    exe = tmp_path / "inflate_model_test"
    src = os.path.join(ROOT, "snap-rnaseq_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", src, "-I", os.path.join(src, "host"),
                    os.path.join(HERE, "c", "inflate_model_test.cpp"), os.path.join(src, "host", "inflate.cpp"),
                    os.path.join(src, "host", "bgzf.cpp"), os.path.join(src, "host", "threads.cpp"), "-o", str(exe),
                    "-lz", "-lpthread"], check=True, capture_output=True)
    out = subprocess.run([str(exe), "3000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and ", 0 failed" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    accepted, refused = map(int, re.search(r"(\d+) damaged members accepted as zlib does, (\d+) refused", out.stdout).groups())
    assert accepted > 0 and refused > 1000      # both branches of the comparison were taken
