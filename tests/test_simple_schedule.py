"""The simple pass's walk schedule (snap-rnaseq_amd/csrc/simple_schedule.h: lowestPossibleScore before and
after every seed step, the step count and the 17th-record flag of an all-ACGT read, from its length alone)
against a transcription of simple_one's seed loop: tests/c/simple_schedule_test.cpp, host code, every read
length for seed lengths 16, 20, 23, 31 and four maxSeeds settings, unlimited and at every score limit."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_schedule_matches_the_seed_loop(tmp_path):
    exe = tmp_path / "simple_schedule_test"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "snap-rnaseq_amd", "csrc"),
                    os.path.join(HERE, "c", "simple_schedule_test.cpp"), "-o", str(exe)], check=True,
                   capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-500:])
    m = re.search(r"(\d+) cases, (\d+) mismatches", out.stdout)
    assert out.returncode == 0 and m and int(m.group(1)) > 20000 and int(m.group(2)) == 0, out.stdout[-2000:]
