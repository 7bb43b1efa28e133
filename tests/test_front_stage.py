"""The front stage of a pass set (counter clear, record pre-fill, pass 0, order_long_kernel, the simple
pass) on its own stream, a chunk or two ahead of the lanes' align kernels, with per-chunk record /
seed / defer buffers and per-pass-set work counters.

Chunk rotation through the four slots, mixed read lengths (passes 2 and 3 launched or skipped),
buffer growth on an open stream and the resident path, each against the oracle and against a
blocking call, under the switches that change the stream layout (SNAPGPU_OVERLAP=0,
SNAPGPU_SIMPLE_PASS=0, SNAPGPU_FRONT_PRIORITY=0)."""
import os

import numpy as np
import pytest

import snapgpu
from oracle_ffi import mismatches, oracle_align

pytestmark = pytest.mark.gpu

SWITCHES = {"default": {}, "overlap0": {"SNAPGPU_OVERLAP": "0"}, "simple0": {"SNAPGPU_SIMPLE_PASS": "0"},
            "frontprio0": {"SNAPGPU_FRONT_PRIORITY": "0"}, "frontprio1": {"SNAPGPU_FRONT_PRIORITY": "1"}}


def _concat(batches):
    return snapgpu.Reads.from_list([b.get(i) for b in batches for i in range(b.n)])


@pytest.fixture(scope="module")
def world(small_world):
    """Read sets on the parity tests' small genome and their oracle records (computed once)."""
    g, idx = small_world["genome"], small_world["index"]
    p = snapgpu.BaseAligner(idx).params
    syn = lambda n, seed, length=100: snapgpu.Reads.synthetic(g, n, seed=seed, read_length=length,
                                                               random_read_fraction=0.01)
    w = {"index": idx, "genome": g}
    w["rot"] = syn(21_000, 15)
    parts = [syn(700, 16), syn(500, 17, 150), syn(300, 18, 300), syn(400, 19), syn(200, 20, 150)]
    w["mixed"] = _concat(parts)
    w["short"] = syn(1500, 21)
    w["grow"] = syn(11_000, 22)
    for k in ("rot", "mixed", "short", "grow"):
        w[k + "_oracle"] = oracle_align(idx, w[k], p, n_threads=8)
    return w


def _same_as_oracle(got, want):
    bad = mismatches(got, want)
    assert len(bad) == 0, f"{len(bad)} reads differ from the oracle, first {bad[:5]}"


def _rotation(w):
    """9 chunks of 2,334 / 2,333 reads over three submits and one wait: every slot is used at least
    twice and the lane alternation wraps."""
    al = snapgpu.BaseAligner(w["index"])   # (SNAPGPU_CHUNK_READS=3000 in the environment)
    reads = w["rot"]
    parts = [reads.slice(s, 7000) for s in (0, 7000, 14000)]
    outs = [np.zeros(7000, dtype=snapgpu.RESULT_DTYPE) for _ in parts]
    for p, o in zip(parts, outs):
        al.submit(p, o)
    al.wait()
    return np.concatenate(outs), al.timing()


def _mixed(w):
    al = snapgpu.BaseAligner(w["index"])
    mixed = al.AlignReads(w["mixed"])
    tm = al.timing()
    short = al.AlignReads(w["short"])
    return mixed, tm, short, al.timing()


def _growth(w):
    al = snapgpu.BaseAligner(w["index"])   # (SNAPGPU_CHUNK_READS=8000 in the environment)
    reads = w["grow"]
    a, b = reads.slice(0, 2000), reads.slice(2000, 9000)
    oa, ob = np.zeros(a.n, dtype=snapgpu.RESULT_DTYPE), np.zeros(b.n, dtype=snapgpu.RESULT_DTYPE)
    al.submit(a, oa)
    al.submit(b, ob)   # two chunks of 4,500 reads: the chunk buffers are reallocated with the stream open
    al.wait()
    return np.concatenate([oa, ob]), al.timing()


def _run_all(w, env):
    """The three stream shapes under the environment switches `env` -> records and timings."""
    keys = list(env) + ["SNAPGPU_CHUNK_READS"]
    saved = {k: os.environ.get(k) for k in keys}
    try:
        os.environ.update(env)
        os.environ["SNAPGPU_CHUNK_READS"] = "3000"
        rot, t_rot = _rotation(w)
        del os.environ["SNAPGPU_CHUNK_READS"]
        whole = snapgpu.BaseAligner(w["index"]).AlignReads(w["rot"])   # one chunk, default chunk size
        mixed, t_mixed, short, t_short = _mixed(w)
        os.environ["SNAPGPU_CHUNK_READS"] = "8000"
        grow, t_grow = _growth(w)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return {"rot": rot, "whole": whole, "mixed": mixed, "short": short, "grow": grow,
            "t_rot": t_rot, "t_mixed": t_mixed, "t_short": t_short, "t_grow": t_grow}


@pytest.fixture(scope="module")
def default_run(world):
    return _run_all(world, {})


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_rotation_mixed_lengths_and_growth(gpu_available, world, default_run, switch):
    r = default_run if switch == "default" else _run_all(world, SWITCHES[switch])
    simple = switch != "simple0"
    lengths = world["mixed"].lengths()
    n_long, n_byte, n_short = int((lengths > 128).sum()), int((lengths > 256).sum()), int((lengths <= 128).sum())
    assert n_long == 1000 and n_byte == 300
    for k in ("t_rot", "t_mixed", "t_short", "t_grow"):
        print(f"{switch} {k}: {r[k]}")

    # rotation
    assert r["rot"].tobytes() == r["whole"].tobytes()
    _same_as_oracle(r["rot"], world["rot_oracle"])
    t = r["t_rot"]
    assert t["nLaunches"] == 9
    assert t["nSimpleReads"] + t["nSimpleBailed"] == (21_000 if simple else 0)
    assert 0 < t["mainKernelBusyMs"] <= t["wallMs"]
    assert t["lookupKernelBusyMs"] > 0

    # mixed lengths: passes 2 and 3 and order_long_kernel run; all 100 bp: they are skipped
    _same_as_oracle(r["mixed"], world["mixed_oracle"])
    _same_as_oracle(r["short"], world["short_oracle"])
    tm, ts = r["t_mixed"], r["t_short"]
    assert (tm["nSpilled"], tm["nByteReads"]) == (n_long, n_byte)
    assert (ts["nSpilled"], ts["nByteReads"]) == (0, 0)
    assert tm["nLaunches"] == 1 and ts["nLaunches"] == 1
    assert tm["nSimpleReads"] + tm["nSimpleBailed"] == (n_short if simple else 0)
    assert ts["nSimpleReads"] + ts["nSimpleBailed"] == (1500 if simple else 0)

    # growth with the stream open
    _same_as_oracle(r["grow"], world["grow_oracle"])
    assert r["t_grow"]["nLaunches"] == 3

    # identical records whatever the switches
    for k in ("rot", "mixed", "short", "grow"):
        assert r[k].tobytes() == default_run[k].tobytes(), f"{k} records differ between default and {switch}"


def test_resident_three_chunks(gpu_available, world):
    """upload / run / results of 600,000 reads (three 2^18-read chunks: the lanes alternate and the
    front stage runs ahead on sub-ranges of the resident buffers) against the host path."""
    reads = snapgpu.Reads.synthetic(world["genome"], 600_000, seed=23)
    al = snapgpu.BaseAligner(world["index"])
    want = al.AlignReads(reads)
    th = al.timing()
    dev = al.upload(reads)
    dev.run()
    got = dev.results()
    tr = al.timing()
    assert got.tobytes() == want.tobytes()
    assert th["nLaunches"] == 1 and tr["nLaunches"] == 3
    assert tr["nSimpleReads"] + tr["nSimpleBailed"] == 600_000
    assert (tr["nSimpleReads"], tr["nSimpleBailed"]) == (th["nSimpleReads"], th["nSimpleBailed"])
    # a second run over the same resident reads, queued behind the first without a synchronise in between
    dev.run()
    dev.run()
    assert dev.results().tobytes() == want.tobytes()
