"""The parallel hash placement of the GPU index builder (snap-rnaseq_amd/csrc/index_place.h) on
the CPU: tests/c/index_place_test.cpp runs the claim loop the device kernel runs, over std::atomic
owner words on 8 threads, and compares every table with sequential insertion."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_claim_loop_matches_sequential_insertion(tmp_path):
    exe = tmp_path / "index_place_test"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "snap-rnaseq_amd", "csrc"),
                    os.path.join(HERE, "c", "index_place_test.cpp"), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe), "6"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout and " 0 overruns" in out.stdout, out.stdout[-2000:]
    assert "overfull table reported: yes" in out.stdout
