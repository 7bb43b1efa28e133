"""The .bai index's host model (snapgpu.bai_build, csrc/host/bai.cpp over csrc/bai_index.h; no GPU):
byte-identical to the plain-Python restatement in bai_cases.py, usable by an independent reader that
queries by region as samtools does, and refusing what the format cannot hold."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import snapgpu
from bai_cases import (D, M, MEMBER, N, brute_force, expected_bai, fabricated, make_record, make_records, parse_bai, query,
                       rec_fields, split)
from bam_cases import permuted

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SLICES = (0, 1, 5, 33, 300)
HEADER = snapgpu.bgzf_compress(b"BAM\1" + bytes(500), eof=False)    # stands for the BGZF of a BAM header


@pytest.fixture(scope="module")
def world_records(small_world):
    """n -> the first n reads of small_world as sorted BAM records (host encoder, host sort keys); the
    locations are the CPU restatement's, every placed read carries one "=" op of its length."""
    from oracle_ffi import oracle_align
    idx, reads = small_world["index"], small_world["reads"]
    res = oracle_align(idx, reads, snapgpu.default_params(), n_threads=8)
    cig = snapgpu.Cigars.empty(reads.n)
    placed = res["location"] != 0xFFFFFFFF
    cig.nOps[placed] = 1
    cig.ops[placed, 0] = (reads.lengths()[placed].astype(np.uint32) << 4) | 7
    ids = [b"read_%d" % i for i in range(reads.n)]
    out = {}
    for n in SLICES + (reads.n,):
        c = snapgpu.Cigars(cig.editDistance[:n], cig.nOps[:n], cig.ops[:n])
        raw, _ = snapgpu.bam_format(idx, reads.slice(0, n), ids[:n], res[:n], c)
        order = np.argsort(snapgpu.bam_sort_keys(idx, res[:n]), kind="stable")
        out[n] = permuted(raw, order)
    return out


def _streams(world_records):
    """name -> (records, n_ref), every stream of this file."""
    s = {"world_%d" % n: (raw, 3) for n, raw in world_records.items()}
    s.update(fabricated())
    return s


def test_small_world_is_what_the_issue_asks_for(world_records):
    raw = world_records[4000]
    refs = {rec_fields(r)["ref"] for r in split(raw)}
    assert refs >= {0, 1, 2} and len(raw) > 10 * MEMBER


@pytest.mark.parametrize("compressor", ["zlib", "model"])
@pytest.mark.parametrize("offset", [0, len(HEADER)])
def test_model_equals_the_restatement(world_records, compressor, offset):
    compress = snapgpu.bgzf_compress if compressor == "zlib" else snapgpu.bgzf_compress_model
    for name, (raw, n_ref) in _streams(world_records).items():
        for eof in (True, False):
            z = compress(raw, eof=eof)
            got = snapgpu.bai_build(raw, z, n_ref, offset)
            assert got == expected_bai(raw, z, n_ref, offset), (name, eof)
            assert len(got) <= snapgpu.lib().snapgpu_bai_size_bound(len(split(raw)), n_ref, len(raw)), name


def test_fabricated_streams_hold_what_they_are_for():
    f = fabricated()
    bai = lambda name: parse_bai(snapgpu.bai_build(f[name][0], snapgpu.bgzf_compress_model(f[name][0]), f[name][1]))
    edges = bai("member_edges")
    cuts = sorted(v for b in edges["refs"][0]["bins"].values() for c in b for v in c)
    assert cuts[0] == 0 and any(v & 0xffff == 0 and v >> 16 for v in cuts)          # a chunk ends on a member's first byte
    assert bai("empty_reference_between")["refs"][1] == dict(bins={}, meta=None, lin=[])
    assert bai("empty_reference_between")["refs"][2]["meta"][1] == (2, 1)
    lin = bai("window_3_only")["refs"][0]["lin"]
    assert len(lin) == 4 and len(set(lin)) == 1                                         # windows 0-2 back-filled
    bins = bai("bins_not_contiguous")["refs"][0]["bins"]
    assert len(bins[4681]) == 2 and len(bins[4681 + 7]) == 2 and 585 in bins and 73 in bins
    lin = bai("long_N")["refs"][0]["lin"]
    assert lin[0] == lin[1] == lin[2] and lin[3] > lin[2]
    assert len(bai("span_1")["refs"][0]["lin"]) == 6
    only = bai("only_unplaced")
    assert only["no_coor"] == 5 and all(r["meta"] is None for r in only["refs"])
    assert bai("equal_pos")["no_coor"] == 2 and bai("equal_pos")["refs"][0]["meta"][1] == (5, 1)


def test_region_queries_return_what_a_scan_returns(world_records):
    rng = np.random.default_rng(19)
    for name, (raw, n_ref) in _streams(world_records).items():
        file_bytes = HEADER + snapgpu.bgzf_compress_model(raw)
        bai = snapgpu.bai_build(raw, file_bytes[len(HEADER):], n_ref, len(HEADER))
        recs = [rec_fields(r) for r in split(raw)]
        found = 0
        for ref in sorted({f["ref"] for f in recs if f["ref"] >= 0}):
            mine = [f for f in recs if f["ref"] == ref]
            top = max(f["end"] for f in mine)
            lin = parse_bai(bai)["refs"][ref]["lin"]
            windows = set(range(len(lin))) - {w for f in mine for w in range(f["pos"] >> 14, ((f["end"] - 1) >> 14) + 1)}
            regions = [(0, top)] + [(w << 14, (w << 14) + 16384) for w in sorted(windows)[:1]]
            for _ in range(20):
                beg = int(rng.integers(0, top))
                regions.append((beg, beg + int(rng.choice([1, 50, 2000, 40000, top]))))
            for k, (beg, end) in enumerate(regions):
                want = brute_force(raw, ref, beg, end)
                assert query(file_bytes, bai, ref, beg, end) == want, (name, ref, beg, end)
                if k == 0:                       # the whole reference
                    found += len(want)
        with_ref = sum(f["ref"] >= 0 for f in recs)
        assert found == with_ref, f"{name}: {found} of {with_ref} records with a refID came back from the whole-reference queries"


def _raises(records, n_ref, what, z=None, offset=0):
    with pytest.raises(snapgpu.SnapGpuError, match=what):
        snapgpu.bai_build(records, snapgpu.bgzf_compress_model(records) if z is None else z, n_ref, offset)


def test_refused_inputs():
    ok = [dict(ref=0, pos=10), dict(ref=0, pos=20), dict(ref=1, pos=5), dict(ref=-1, pos=-1, cigar=())]
    good = make_records(ok)
    snapgpu.bai_build(good, snapgpu.bgzf_compress_model(good), 2)
    first = len(make_record(**ok[0]))
    _raises(good[:-3], 2, r"record 3: truncated")
    _raises(good[:first + 2], 2, r"record 1: truncated")
    short = bytearray(make_record(0, 30, cigar=((5, M), (5, D))))
    short[0:4] = (len(short) - 4 - 6).to_bytes(4, "little")              # its CIGAR passes its end
    _raises(good[:first] + bytes(short[:-6]), 2, r"record 1: truncated")
    at2 = lambda bad: ok[:2] + [bad] + ok[2:]
    for specs, k, why in ((at2(dict(ref=2, pos=5)), 2, "refID"), (at2(dict(ref=-2, pos=5)), 2, "refID"),
                          (at2(dict(ref=1, pos=-1)), 2, "pos < 0"),
                          (at2(dict(ref=1, pos=(1 << 29) - 10, cigar=((11, M),))), 2, "2\\^29"),
                          (at2(dict(ref=0, pos=19)), 2, "order"),                        # pos goes down
                          ([ok[0], ok[2], ok[1], ok[3]], 2, "order"),                    # refID goes down
                          ([ok[0], ok[3], ok[1], ok[2]], 2, "order")):                   # a refID after -1
        _raises(make_records(specs), 2, r"record %d: .*%s" % (k, why))
    edge = make_records([dict(ref=1, pos=(1 << 29) - 10, cigar=((10, N),))])  # ends exactly at 2^29
    assert len(parse_bai(snapgpu.bai_build(edge, snapgpu.bgzf_compress_model(edge), 2))["refs"][1]["lin"]) == 1 << 15
    _raises(good, 2, "ISIZE", z=snapgpu.bgzf_compress_model(good + b"x"))
    _raises(good, 2, "streamOffset", offset=1 << 48)
    snapgpu.bai_build(good, snapgpu.bgzf_compress_model(good), 2, (1 << 48) - 1)


def test_a_cap_too_small_reports_the_size_needed():
    raw, n_ref = fabricated()["equal_pos"]
    z = snapgpu.bgzf_compress_model(raw)
    want = snapgpu.bai_build(raw, z, n_ref)
    buf, used = C.create_string_buffer(len(want)), C.c_uint64()
    fn = snapgpu.lib().snapgpu_bai_build
    assert fn(raw, len(raw), n_ref, z, len(z), 0, buf, len(want) - 1, C.byref(used)) == -1 and used.value == len(want)
    assert fn(raw, len(raw), n_ref, z, len(z), 0, None, 0, C.byref(used)) == -1 and used.value == len(want)
    assert fn(raw, len(raw), n_ref, z, len(z), 0, buf, len(want), C.byref(used)) == 0 and buf.raw == want


def test_stand_alone_program_under_sanitizers(tmp_path):
    """tests/c/bai_model_test.cpp: the model's sources with -fsanitize=address,undefined in a program of their
    own, over 2,000 seeded random sorted streams, each in a buffer of exactly its size, and their truncated forms."""
    exe = tmp_path / "bai_model_test"
    src = os.path.join(ROOT, "snap-rnaseq_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", src, "-I", os.path.join(src, "host"),
                    os.path.join(HERE, "c", "bai_model_test.cpp"), os.path.join(src, "host", "bai.cpp"),
                    os.path.join(src, "host", "bgzf.cpp"), os.path.join(src, "host", "inflate.cpp"),
                    os.path.join(src, "host", "threads.cpp"), "-o", str(exe), "-lz", "-lpthread"],
                   check=True, capture_output=True)
    out = subprocess.run([str(exe), "2000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and ", 0 failed" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    built, refused = map(int, re.search(r"(\d+) streams indexed, (\d+) truncated forms refused", out.stdout).groups())
    assert built == 2000 and refused > 1000
