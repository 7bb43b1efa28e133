"""BGZF streams shared by test_inflate_model.py and test_inflate_gpu.py.  The good ones carry their
expected bytes from Python's zlib / gzip, never from the code under test; the bad ones are each
refused by zlib (checked when they are built).  zlib itself never writes a 15-bit code or the
farther distances, so two members are written by hand: dynamic_block() below."""
import gzip
import os
import re
import zlib

import numpy as np

from bgzf_cases import BLOCK, EOF_BLOCK, GOLDEN, SIZED

EFORMAT = -5   # SNAPGPU_EFORMAT (include/snapgpu.h)
EINVAL = -1

# inflate_block.h's Status values the fixed bad cases meet
ST = {"block_type": 1, "stored_length": 2, "no_eob": 6, "lit_over": 7, "lit_incomplete": 8, "length_symbol": 12,
      "distance_symbol": 13, "distance_too_far": 14, "output_overflow": 15, "exhausted": 16, "size": 18, "crc": 19}


GOOD = ["empty", "eof_only", "one_byte", "empty_between", "stored_level0", "random_level6", "fixed", "huffman_only", "rle",
        "mem_level1", "full_flush", "max_isize", "zeros", "period3", "period259", "long15", "overlap", "extra_subfield",
        "fq_level1", "fq_level6", "fq_level9", "fq_block1000"]                         # good()'s names
BAD = ["dist_before_start", "oversubscribed", "incomplete_ll", "truncated", "stored_nlen", "btype3", "no_eob",
       "fixed_dist30", "fixed_len286", "crc", "isize_plus", "isize_minus"]             # bad_members()'s
CONTAINERS = ["magic", "flg0", "no_bc", "bsize_past_end", "trailing", "isize_65537"]   # bad_containers()'s


def refusal(fn, stream):
    """(return code, member index, status or None) of the SnapGpuError fn raises on `stream`."""
    import pytest
    import snapgpu
    with pytest.raises(snapgpu.SnapGpuError) as e:
        fn(stream)
    text = str(e.value)
    code = int(re.search(r"failed \((-?\d+)\)", text).group(1))
    where = re.search(r"member (\d+) at byte (\d+)", text)
    status = re.search(r"\(status (\d+)\)", text)
    return code, int(where.group(1)) if where else None, int(status.group(1)) if status else None


def member(deflate, data, crc=None, isize=None, extra=b""):
    """One BGZF member around the raw deflate bytes; extra: subfields ahead of BC."""
    xlen = len(extra) + 6
    size = 12 + xlen + len(deflate) + 8
    assert size <= 65536
    crc = zlib.crc32(data) if crc is None else crc
    isize = len(data) if isize is None else isize
    return (bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255]) + xlen.to_bytes(2, "little") + extra + b"BC\x02\x00" +
            (size - 1).to_bytes(2, "little") + deflate + crc.to_bytes(4, "little") + isize.to_bytes(4, "little"))


def deflate_of(piece, level=6, strategy=0, mem_level=8, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    if flush_at is None:
        return c.compress(piece) + c.flush()
    return c.compress(piece[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(piece[flush_at:]) + c.flush()


def bgzf(data, level=6, strategy=0, mem_level=8, block=BLOCK, flush_at=None):
    """`data` in members of `block` bytes, each compressed by zlib; header and trailer written here."""
    return b"".join(member(deflate_of(data[k:k + block], level, strategy, mem_level, flush_at), data[k:k + block])
                    for k in range(0, len(data), block))


# ---------------------------------------------------------------- one block by hand
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, bits):          # low bit first
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, bits):         # a Huffman code: top bit first
        self.put(int(format(value, "0%db" % bits)[::-1], 2) if bits else 0, bits)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lens):
    """RFC 1951 3.2.2: symbol -> code, for any lengths (an over-subscribed set still gets numbers)."""
    code, codes = 0, {}
    for bits in range(1, 16):
        for sym, l in enumerate(lens):
            if l == bits:
                codes[sym] = code
                code += 1
        code <<= 1
    return codes


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
              6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def _sym_of(value, base):
    return max(s for s in range(len(base)) if base[s] <= value)


def lens(n, **by_symbol):
    """lens(288, s97=2, s256=3): code lengths with the named symbols set."""
    out = [0] * n
    for k, l in by_symbol.items():
        out[int(k[1:])] = l
    return out


def one_block(tokens, lit_lens, dist_lens, btype=2, eob=True):
    """A final block of the tokens: an int is a literal, (length, distance) a match, ("L", s) the bare
    literal/length symbol s, ("D", length, s) a length followed by the bare distance symbol s.
    btype 2 writes the code lengths one by one through a code-length code of 4 bits for 0 .. 15."""
    w = Bits()
    w.put(1, 1)
    w.put(btype, 2)
    if btype == 2:
        hlit = max(257, max(i for i, l in enumerate(lit_lens) if l) + 1)
        hdist = max(1, max([i for i, l in enumerate(dist_lens) if l] or [0]) + 1)
        w.put(hlit - 257, 5)
        w.put(hdist - 1, 5)
        w.put(19 - 4, 4)
        for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
            w.put(4 if s < 16 else 0, 3)
        for l in list(lit_lens[:hlit]) + list(dist_lens[:hdist]):
            w.code(l, 4)                 # 16 codes of 4 bits: the code of l is l
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for t in list(tokens) + ([("L", 256)] if eob else []):
        if isinstance(t, int):
            w.code(lit[t], lit_lens[t])
        elif t[0] == "L":
            w.code(lit[t[1]], lit_lens[t[1]])
        else:
            length = t[1] if t[0] == "D" else t[0]
            s = _sym_of(length, _LEN_BASE)
            w.code(lit[257 + s], lit_lens[257 + s])
            w.put(length - _LEN_BASE[s], _LEN_EXTRA[s])
            if t[0] == "D":
                w.code(dist[t[2]], dist_lens[t[2]])
            else:
                s = _sym_of(t[1], _DIST_BASE)
                w.code(dist[s], dist_lens[s])
                w.put(t[1] - _DIST_BASE[s], _DIST_EXTRA[s])
    return w.bytes()


def zlib_inflates(deflate):
    """What zlib makes of the raw stream: its bytes, or None when it refuses or wants more."""
    z = zlib.decompressobj(-15)
    try:
        out = z.decompress(deflate) + z.flush()
    except zlib.error:
        return None
    return out if z.eof and z.unused_data == b"" else None


def _by_hand(deflate):
    data = zlib_inflates(deflate)
    assert data is not None
    return member(deflate, data), data


def long15():
    lit = lens(288, **{"s%d" % i: i + 1 for i in range(14)}, s14=15, s256=15)
    return one_block(list(range(15)) * 3 + [14, 0, 13, 14], lit, [1])


def overlap():
    lit = lens(288, s97=2, s98=2, s99=3, s256=3, s277=3, s285=3)
    dist = lens(30, s0=2, s1=2, s2=2, s11=3, s12=3)
    return one_block([97, 98, 99, (258, 1), (258, 2), (258, 3), (70, 63), (70, 64), (70, 65)], lit, dist)


def _random(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def fastq_text():
    return open(os.path.join(GOLDEN, "single_reads.fq"), "rb").read()


_good = None


def good():
    """name -> (BGZF stream, the bytes it inflates to); built once, never modified."""
    global _good
    if _good is not None:
        return _good
    fq = fastq_text()
    g = {"empty": (b"", b""), "eof_only": (EOF_BLOCK, b""), "one_byte": (bgzf(b"Q"), b"Q")}
    g["empty_between"] = (bgzf(b"abc") + EOF_BLOCK + bgzf(b"def" * 100) + EOF_BLOCK + EOF_BLOCK + bgzf(b"x"),
                          b"abc" + b"def" * 100 + b"x")
    for name, data, kw in [("stored_level0", _random(BLOCK, 1), dict(level=0)),
                           ("random_level6", _random(BLOCK, 2), {}),
                           ("fixed", fq[:BLOCK], dict(strategy=zlib.Z_FIXED)),
                           ("huffman_only", fq[:BLOCK], dict(strategy=zlib.Z_HUFFMAN_ONLY)),
                           ("rle", fq[:BLOCK], dict(strategy=zlib.Z_RLE)),
                           ("mem_level1", fq[:BLOCK], dict(mem_level=1)),
                           ("full_flush", fq[:BLOCK], dict(flush_at=30000)),
                           ("max_isize", fq[:65536], dict(block=65536)),
                           ("zeros", SIZED["zeros"](BLOCK), {}), ("period3", SIZED["period3"](BLOCK), {}),
                           ("period259", SIZED["period259"](BLOCK), {}),
                           ("fq_level1", fq, dict(level=1)), ("fq_level6", fq, {}), ("fq_level9", fq, dict(level=9)),
                           ("fq_block1000", fq[:40000], dict(block=1000))]:
        g[name] = (bgzf(data, **kw), data)
    assert len(fq) >= 65536 and len(g["max_isize"][0]) <= 65536
    g["long15"] = _by_hand(long15())
    g["overlap"] = _by_hand(overlap())
    assert len(g["overlap"][1]) == 987
    body = deflate_of(b"extra field first")
    g["extra_subfield"] = (member(body, b"extra field first", extra=b"XY\x03\x00abc"), b"extra field first")
    for name, (stream, data) in g.items():
        assert (gzip.decompress(stream) if stream else b"") == data, name
    _good = g
    return g


_bad = None


def bad_members():
    """name -> (one member zlib refuses, the Status inflate_block.h gives it)."""
    global _bad
    if _bad is not None:
        return _bad
    a, b_ = 97, 98
    ok_data = fastq_text()[:5000]
    ok = deflate_of(ok_data)
    streams = {
        "dist_before_start": (one_block([a, (70, 2)], lens(288, s97=1, s256=2, s277=2), [0, 1]), ST["distance_too_far"]),
        "oversubscribed": (one_block([a], lens(288, s97=1, s98=1, s256=1), [1]), ST["lit_over"]),
        "incomplete_ll": (one_block([a], lens(288, s97=2, s256=2), [1]), ST["lit_incomplete"]),
        "truncated": (ok[:len(ok) // 2], ST["exhausted"]),
        "stored_nlen": (bytes([1, 5, 0, 0xfa, 0xfe]) + b"hello", ST["stored_length"]),
        "btype3": (bytes([7, 0]), ST["block_type"]),
        "no_eob": (one_block([a, b_], lens(288, s97=1, s98=1), [1], eob=False), ST["no_eob"]),
        "fixed_dist30": (one_block([a, ("D", 3, 30)], FIXED_LIT, FIXED_DIST, btype=1), ST["distance_symbol"]),
        "fixed_len286": (one_block([a, ("L", 286)], FIXED_LIT, FIXED_DIST, btype=1), ST["length_symbol"]),
    }
    out = {}
    for name, (deflate, status) in streams.items():
        assert zlib_inflates(deflate) is None, name
        out[name] = (member(deflate, ok_data if name == "truncated" else b"a"), status)
    out["crc"] = (member(ok, ok_data, crc=zlib.crc32(ok_data) ^ 1), ST["crc"])
    out["isize_plus"] = (member(ok, ok_data, isize=len(ok_data) + 1), ST["size"])
    out["isize_minus"] = (member(ok, ok_data, isize=len(ok_data) - 1), ST["output_overflow"])
    _bad = out
    return out


def bad_containers():
    """name -> a stream the member walk refuses at member 1 (a good member comes first)."""
    first = bgzf(b"a good member")
    m = bgzf(b"second member")
    big = bytearray(m)
    big[-4:] = (65537).to_bytes(4, "little")
    return {
        "magic": first + b"\x1f\x8c" + m[2:],
        "flg0": first + gzip.compress(b"plain gzip"),
        "no_bc": first + m[:12] + b"XY" + m[14:],
        "bsize_past_end": first + m[:-3],
        "trailing": first + b"\0\0\0",
        "isize_65537": first + bytes(big),
    }


def placed(bad, where, n=5):
    """n members, good ones but for the bad member(s) at the indices `where`."""
    fill = [bgzf(b"member %d " % k * 50) for k in range(n)]
    for k in where:
        fill[k] = bad
    return b"".join(fill)
