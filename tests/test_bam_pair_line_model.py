"""csrc/bam_pair_line.h in a stand-alone host program under AddressSanitizer and UBSan (no GPU)."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """tests/c/bam_pair_line_test.cpp: the pair record rule with the Serial group, built with
    -fsanitize=address,undefined in a program of its own, over 400 seeded random pair batches whose
    reads and ids live in heap blocks of exactly their sizes and whose records are written into a
    buffer of exactly their summed sizes between guard bytes."""
    exe = tmp_path / "bam_pair_line_test"
    src = os.path.join(ROOT, "snap-rnaseq_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", src,
                    os.path.join(HERE, "c", "bam_pair_line_test.cpp"), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe), "400"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and ", 0 failed" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    batches, records, carried = map(int, re.search(r"(\d+) batches, (\d+) records, (\d+) carried", out.stdout).groups())
    assert batches == 400 and records > 10000 and carried > 1000
