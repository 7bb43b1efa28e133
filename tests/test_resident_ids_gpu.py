"""SAM, BAM and BGZF from a device-parsed batch without a host batch: run_sam(None) / run_bam(None) on
what upload_fastq(host_batch=False) leaves resident (ids, clip arrays, the tail past the largest clipped
end), and DeviceReads.ids().  Every expected value is the host-batch chain on the same input: host
parser -> clip -> upload -> run -> run_cigars -> run_sam(reads) / run_bam(reads) / run_bgzf."""
import ctypes as C

import numpy as np
import pytest

import snapgpu
from fastq_cases import CASES, _B60, _q, batch_fields, host_batch, random_text, rec

pytestmark = pytest.mark.gpu

EINVAL = -1   # include/snapgpu.h
EOF_BLOCK = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
CLIP_MESSAGE = "sam_format: nOps > SNAPGPU_CIGAR_MAX_OPS, read longer than 1024 bases or bad clip arrays"
ID_MESSAGE = "bam_format: a read id is longer than 254 bytes"
KEYS = ("sam", "sam_sorted", "sam_order", "bam", "bam_carry", "bam_sorted", "bam_order", "bgzf")


@pytest.fixture(scope="module")
def world(gpu_available, small_world, tmp_path_factory):
    """small_world's 4,000 reads as FASTQ text: every seventh read and the last with '#' runs of 5 and 8
    at the ends, every fifth id with words after a space (the SAM QNAME stops there, the BAM one does not)."""
    al = snapgpu.BaseAligner(small_world["index"])
    tmp = tmp_path_factory.mktemp("resident_ids")
    path = tmp / "reads.fq"
    small_world["reads"].write_fastq(path)
    lines = path.read_bytes().split(b"\n")
    for r in list(range(0, 4000, 7)) + [3999]:
        q = lines[4 * r + 3]
        lines[4 * r + 3] = b"#" * 5 + q[5:-8] + b"#" * 8
    for r in range(0, 4000, 5):
        lines[4 * r] += b" extra words"
    text = b"\n".join(lines)
    path.write_bytes(text)
    gz = tmp / "reads.fq.gz"
    gz.write_bytes(snapgpu.bgzf_compress(text))
    return {"al": al, "idx": small_world["index"], "path": path, "gz": gz, "text": text, "lines": lines}


def format_all(dev, reads):
    """Every output of the formatters for one aligned batch; reads = None: from the resident state."""
    out = {}
    dev.run_sam(reads)
    out["sam"] = dev.sam()
    dev.run_sam(reads, sorted_output=True)
    out["sam_sorted"], out["sam_order"] = dev.sam(), dev.sam_order().tobytes()
    dev.run_bam(reads, nm_carry=7)
    out["bam"], out["bam_carry"] = dev.bam(), dev.bam_nm_carry()
    dev.run_bam(reads, sorted_output=True, nm_carry=7)
    out["bam_sorted"], out["bam_order"] = dev.bam(), dev.bam_order().tobytes()
    dev.run_bgzf()
    out["bgzf"] = dev.bgzf()
    return out


def aligned(dev):
    dev.run()
    dev.run_cigars()
    return dev


def host_chain(al, text, clipping):
    reads = host_batch(text, clipping)
    return format_all(aligned(al.upload(reads)), reads)


def assert_same_outputs(got, want, what):
    for k in KEYS:
        assert got[k] == want[k], f"{what}: {k} differs"


@pytest.mark.parametrize("clipping", [0, 1, 2, 3])
def test_chain(world, clipping):
    al = world["al"]
    want = host_chain(al, world["text"], clipping)
    assert want["sam"].count(b"\n") == 4000 and want["sam"] != want["sam_sorted"]
    assert b" extra words" in want["bam"] and b" extra words" not in want["sam"]
    for source, bgzf in ((world["path"], False), (world["gz"], True)):
        dev = al.upload_fastq(source, clipping=clipping, host_batch=False, bgzf=bgzf)
        assert dev.reads is None and dev.n == 4000
        # a tail exists exactly when the back clip of the last read was applied
        assert (dev.peek(arrays=False)["bytes"] < 400000) == (clipping in (2, 3))
        assert_same_outputs(format_all(aligned(dev), None), want, f"clipping {clipping}, bgzf {bgzf}")


def test_lifetime(world):
    """A's resident ids survive the next upload_fastq on the aligner, which reuses the parser's buffers."""
    al, lines = world["al"], world["lines"]
    text_a = b"\n".join(lines[:4 * 600]) + b"\n"
    text_b = b"\n".join(l + b"/B" if k % 4 == 0 else l for k, l in enumerate(lines[4 * 1000:4 * 1900])) + b"\n"
    want_a, want_b = host_chain(al, text_a, 3), host_chain(al, text_b, 3)
    a = al.upload_fastq(text_a, clipping=3, host_batch=False)
    b = al.upload_fastq(text_b, clipping=3, host_batch=False)
    assert (a.n, b.n) == (600, 900)
    assert_same_outputs(format_all(aligned(a), None), want_a, "A after B was uploaded")
    assert_same_outputs(format_all(aligned(b), None), want_b, "B")
    assert a.ids()[0] == [l[1:] for l in lines[:4 * 600:4]]


_R = lambda k, q: rec(b"read%d some words" % k, _B60, q)
TAILS = {
    "last_back_clipped": _R(0, _q(0, 60, 0)) + _R(1, _q(3, 57, 0)) + _R(2, _q(0, 51, 9)),
    "last_front_only": _R(0, _q(0, 52, 8)) + _R(1, _q(7, 53, 0)),
    "last_unclipped": _R(0, _q(4, 50, 6)) + _R(1, _q(0, 60, 0)),
    "last_all_hash": _R(0, _q(2, 55, 3)) + _R(1, b"#" * 60),
    "clip_leaves_50": CASES["clip_leaves_50"],
    "clip_back_only": CASES["clip_back_only"],
}


@pytest.mark.parametrize("name", sorted(TAILS))
def test_tail(world, name):
    """The bases and qualities past the largest clipped end come from the resident tail, not a host batch."""
    al = world["al"]
    for clipping in (0, 1, 2, 3):
        full = aligned(al.upload_fastq(TAILS[name], clipping=clipping, host_batch=True))
        bare = aligned(al.upload_fastq(TAILS[name], clipping=clipping, host_batch=False))
        full.run_sam(full.reads)
        bare.run_sam(None)
        want = full.sam()
        assert bare.sam() == want and want.count(b"\n") == full.n, (name, clipping)
        for line in want.splitlines():                       # the whole unclipped read is printed
            assert len(line.split(b"\t")[9]) == 60
        full.run_bam(full.reads)
        bare.run_bam(None)
        assert bare.bam() == full.bam(), (name, clipping)
        # and on the batch that has a host batch too, from its own resident state
        full.run_sam(None)
        assert full.sam() == want, (name, clipping)


def test_alternation(world):
    """Host-form and device-form calls on one batch: the cached aux upload never serves the other form."""
    al = world["al"]
    text = b"\n".join(world["lines"][:4 * 700]) + b"\n"
    dev = aligned(al.upload_fastq(text, clipping=3, host_batch=True))
    reads = dev.reads
    clip = (batch_fields(reads)["frontClipped"], batch_fields(reads)["unclippedLength"])
    res, cig = dev.results(), dev.cigars()
    want = {rg: snapgpu.sam_format(world["idx"], reads, reads.ids(), res, cig, read_group=rg, clip=clip)
            for rg in ("FASTQ", None)}
    assert want["FASTQ"] != want[None]
    for r, rg in ((reads, "FASTQ"), (None, "FASTQ"), (reads, "FASTQ"), (None, None), (None, "FASTQ"), (reads, None)):
        dev.run_sam(r, read_group=rg)
        assert dev.sam() == want[rg], (r is None, rg)
    dev.run_sam(None, ids=reads.ids())                        # caller ids with reads = None go up as before
    assert dev.sam() == want["FASTQ"]


def raw_ids(dev):
    """snapgpu_device_reads_ids_download's arrays as they come."""
    fn, n = snapgpu.lib().snapgpu_device_reads_ids_download, dev.n
    used = C.c_uint64()
    rc = fn(dev.aligner._h, dev._h, None, 0, C.byref(used), None, None, None, None)
    assert rc == (EINVAL if used.value else 0)               # the size contract of snapgpu_sam_download
    blob = np.zeros(used.value + 1, np.uint8)
    off, ln = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint32)
    front, full = np.full(n + 1, 77, np.uint32), np.full(n + 1, 77, np.uint32)
    assert fn(dev.aligner._h, dev._h, blob.ctypes.data, used.value, C.byref(used), off.ctypes.data, ln.ctypes.data,
              front.ctypes.data, full.ctypes.data) == 0
    return blob[:used.value].tobytes(), off[:n], ln[:n], front[:n], full[:n]


@pytest.mark.parametrize("clipping", [0, 3])
def test_ids(world, clipping):
    al = world["al"]
    text = random_text(18, 300)
    want = batch_fields(host_batch(text, clipping))
    dev = al.upload_fastq(text, clipping=clipping, host_batch=False)
    al.upload_fastq(CASES["crlf"], host_batch=False)          # the parser's buffers move on
    blob, off, ln, front, full = raw_ids(dev)
    assert blob == want["ids"]
    assert np.array_equal(off, want["idOffsets"]) and np.array_equal(ln, want["idLengths"])
    if clipping:
        assert np.array_equal(front, want["frontClipped"]) and np.array_equal(full, want["unclippedLength"])
        assert front.any() and (full > 0).any()
    else:
        assert (front == 77).all() and (full == 77).all()    # left untouched
    ids, f, u = dev.ids()
    assert ids == [blob[int(o):int(o) + int(l)] for o, l in zip(off, ln)] and len(ids) == want["n"]
    if clipping:
        assert np.array_equal(f, front) and np.array_equal(u, full)
    else:
        assert f is None and u is None


def test_empty_text(world):
    dev = world["al"].upload_fastq(b"", clipping=3, host_batch=False)
    assert dev.n == 0 and dev.ids() == ([], None, None)
    dev.run_cigars()
    dev.run_sam(None)
    assert dev.sam() == b""
    dev.run_bam(None)
    assert dev.bam() == b""
    dev.run_bgzf()
    assert dev.bgzf() == EOF_BLOCK


def refused(call, message):
    with pytest.raises(snapgpu.SnapGpuError) as e:
        call()
    assert f"({EINVAL})" in str(e.value) and message in str(e.value), str(e.value)


def test_refusals(world):
    al = world["al"]
    text = b"\n".join(world["lines"][:4 * 50]) + b"\n"
    up = aligned(al.upload(host_batch(text, 3)))
    refused(lambda: up.run_sam(None), "holds no ids or clip state of its own")
    refused(lambda: up.run_bam(None), "holds no ids or clip state of its own")
    refused(up.ids, "holds no ids of its own")
    dev = al.upload_fastq(text, clipping=3, host_batch=False)
    dev.run()
    refused(lambda: dev.run_sam(None), "no snapgpu_cigar_resident before snapgpu_sam_resident")
    refused(lambda: dev.run_bam(None), "no snapgpu_cigar_resident before snapgpu_bam_resident")
    dev.synchronize()
    long_read = rec(b"a", _B60, b"I" * 60) + rec(b"long", b"ACGTA" * 205, b"I" * 1025)
    dev = al.upload_fastq(long_read, clipping=3, host_batch=False)
    refused(lambda: dev.run_sam(None), CLIP_MESSAGE)
    refused(lambda: dev.run_bam(None), CLIP_MESSAGE)


@pytest.mark.parametrize("id_len", [254, 255])
def test_id_limit(world, id_len):
    al = world["al"]
    text = rec(b"a", _B60, _q(0, 55, 5)) + rec(b"i" * id_len, _B60, b"I" * 60) + rec(b"z", _B60, _q(5, 55, 0))
    full = aligned(al.upload_fastq(text, clipping=3, host_batch=True))
    bare = aligned(al.upload_fastq(text, clipping=3, host_batch=False))
    full.run_sam(full.reads)
    bare.run_sam(None)
    assert bare.sam() == full.sam() and b"i" * id_len in full.sam()
    if id_len > 254:
        refused(lambda: full.run_bam(full.reads), ID_MESSAGE)
        refused(lambda: bare.run_bam(None), ID_MESSAGE)
    else:
        full.run_bam(full.reads)
        bare.run_bam(None)
        assert bare.bam() == full.bam() and b"i" * id_len in full.bam()
