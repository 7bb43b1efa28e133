"""Inputs and checks shared by test_bgzf_model.py and test_bgzf_gpu.py: the block compressor of
snap-rnaseq_amd/csrc/bgzf_block.h writes BGZF members that are not zlib's, so every expected value
comes from the format itself and from Python's zlib / gzip as the inflater."""
import gzip
import os
import zlib

import numpy as np

BLOCK = 0xff00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")   # test_bam_host.py pins it
HEADER16 = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SIZES = (0, 1, 2, 3, 4, 257, 258, 259, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 5)


def _period(k):
    unit = bytes((37 * i + i // 7 + 1) & 0xff for i in range(k))
    return lambda n: (unit * (n // k + 1))[:n]


def _random(n):
    return np.random.default_rng(1000 + n).integers(0, 256, size=n, dtype=np.uint8).tobytes()


SIZED = {"zeros": lambda n: bytes(n), "period2": _period(2), "period3": _period(3), "period259": _period(259),
         "random": _random}


def de_bruijn_16_4():
    """65,536 bytes over 16 values in which no 4 consecutive bytes occur twice: Huffman shortens them to
    half, and no match is possible inside them."""
    k, n = 16, 4
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(seq)


def _motif_at(filler, *offsets):
    motif = (np.random.default_rng(40).integers(0, 64, size=40, dtype=np.uint8) + 128).tobytes()
    d = bytearray(filler)
    for o in offsets:
        d[o:o + 40] = motif
    return bytes(d)


def _fibonacci():
    counts, a, b = [], 1, 1
    while sum(counts) + a <= BLOCK:
        counts.append(a)
        a, b = b, a + b
    counts.append(BLOCK - sum(counts))
    d = np.repeat(np.arange(len(counts), dtype=np.uint8), counts)
    np.random.default_rng(5).shuffle(d)
    return d.tobytes()


def golden_records(name):
    return gzip.open(os.path.join(GOLDEN, name + ".bam.records.gz")).read()


_special = None


def special():
    """name -> bytes, built once and never modified."""
    global _special
    if _special is None:
        filler = de_bruijn_16_4()
        _special = {
            "one_byte_1": b"Q", "one_byte_2": b"QQ",
            "all_256_once": np.random.default_rng(256).permutation(256).astype(np.uint8).tobytes(),
            "motif_32768": _motif_at(filler[:BLOCK], 0, 32768),       # the farthest distance deflate has
            "motif_32769": _motif_at(filler[:BLOCK], 0, 32769),       # one beyond it
            "motif_across_blocks": _motif_at(filler[:BLOCK] + filler[:3000], BLOCK - 40, BLOCK),
            "fibonacci": _fibonacci(),
            "rna_paired": golden_records("expected_rna_paired"),
            "single": golden_records("expected_single"),
        }
    return _special


def members(stream):
    """[(start, size)] of the members of a BGZF stream, by their BSIZE fields."""
    out, at = [], 0
    while at < len(stream):
        assert stream[at:at + 16] == HEADER16, at
        size = int.from_bytes(stream[at + 16:at + 18], "little") + 1
        out.append((at, size))
        at += size
    assert at == len(stream)
    return out


def btype(stream, start):
    return (stream[start + 18] >> 1) & 3


def check_stream(out, data, eof):
    """Everything the format promises about `out` as the BGZF stream of `data`."""
    assert gzip.decompress(out) == data if out else data == b""
    mem = members(out)
    n_blocks = (len(data) + BLOCK - 1) // BLOCK
    assert len(mem) == n_blocks + (1 if eof else 0)
    if eof:
        assert out[-28:] == EOF_BLOCK
    for k in range(n_blocks):
        at, size = mem[k]
        piece = data[k * BLOCK:(k + 1) * BLOCK]
        assert size <= len(piece) + 31
        assert int.from_bytes(out[at + size - 8:at + size - 4], "little") == zlib.crc32(piece)
        assert int.from_bytes(out[at + size - 4:at + size], "little") == len(piece)
        z = zlib.decompressobj(-15)          # alone: a match into the previous block would fail here
        assert z.decompress(out[at + 18:at + size - 8]) + z.flush() == piece
        assert z.eof and z.unused_data == b""
    return mem
