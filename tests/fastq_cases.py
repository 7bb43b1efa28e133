"""FASTQ texts for the parser tests (host buffer form, stand-alone program, device parser), a pure-Python
restatement of the record rule (csrc/fastq_record.h), and the field-by-field comparison of two host
batches over the ctypes struct."""
import ctypes as C
import random

import numpy as np

import snapgpu


# ------------------------------------------------------------------ the rule, restated
def py_parse(text):
    """-> [(id, bases, qualities padded / cut to the bases)] or None for a record without '@' header."""
    lines = text.split(b"\n")
    if lines[-1] == b"":          # nothing follows the last newline; a last line without one counts
        lines.pop()
    trim = lambda l: l.split(b"\0")[0].rstrip(b"\r\n")
    recs = []
    for r in range(len(lines) // 4):   # 1-3 trailing lines are ignored
        h, b, q = trim(lines[4 * r]), trim(lines[4 * r + 1]), trim(lines[4 * r + 3])
        if not h.startswith(b"@"):
            return None
        recs.append((h[1:], b, q[:len(b)].ljust(len(b), b"\0")))
    return recs


def py_clip(q, clipping):
    """Read::clip -> (front, clipped length)."""
    full = ln = len(q)
    front = 0
    if clipping in (2, 3):
        ln = len(q.rstrip(b"#"))
    if clipping in (1, 3):
        while front < ln and q[front:front + 1] == b"#":
            front += 1
    return (0, full) if ln - front < 50 else (front, ln - front)


def py_batch(text, clipping):
    """The fields batch_fields() gives for the host parser's batch clipped at `clipping`, or None."""
    recs = py_parse(text)
    if recs is None:
        return None
    n = len(recs)
    full = np.array([len(b) for _, b, _ in recs], dtype=np.uint32).reshape(n)
    start = np.concatenate([[0], np.cumsum(full, dtype=np.uint64)]).astype(np.uint64)
    clips = [py_clip(q, clipping) for _, _, q in recs]
    front = np.array([c[0] for c in clips], dtype=np.uint32).reshape(n)
    idlen = np.array([len(i) for i, _, _ in recs], dtype=np.uint32).reshape(n)
    total = int(start[n])
    return {
        "n": n, "totalBytes": total,
        "offsets": start[:n] + front, "lengths": np.array([c[1] for c in clips], dtype=np.uint32).reshape(n),
        "bases": b"".join(b for _, b, _ in recs) + bytes(64), "quals": b"".join(q for _, _, q in recs) + bytes(64),
        "ids": b"".join(i for i, _, _ in recs),
        "idOffsets": np.concatenate([[0], np.cumsum(idlen, dtype=np.uint64)]).astype(np.uint64)[:n], "idLengths": idlen,
        "frontClipped": front if clipping else None, "unclippedLength": full if clipping else None,
        "clipping": clipping,
    }


# ------------------------------------------------------------------ batches over the ctypes struct
def _arr(ptr, n, dtype):
    if not ptr:
        return None
    return np.ctypeslib.as_array(ptr, shape=(max(1, n),))[:n].astype(dtype, copy=True)


def batch_fields(reads):
    """Every field of a host batch (snapgpu.Reads) that the parsers define, as plain values."""
    r = reads._p.contents
    n = r.n
    idlen = _arr(r.idLengths, n, np.uint32)
    idoff = _arr(r.idOffsets, n, np.uint64)
    id_bytes = int((idoff + idlen).max()) if n else 0
    return {
        "n": n, "totalBytes": r.totalBytes,
        "offsets": _arr(r.offsets, n, np.uint64), "lengths": _arr(r.lengths, n, np.uint32),
        "bases": C.string_at(r.bases, r.totalBytes + 64), "quals": C.string_at(r.quals, r.totalBytes + 64),
        "ids": C.string_at(r.ids, id_bytes), "idOffsets": idoff, "idLengths": idlen,
        "frontClipped": _arr(r.frontClipped, n, np.uint32), "unclippedLength": _arr(r.unclippedLength, n, np.uint32),
        "clipping": r.clipping, "nUploads": r.nUploads,
    }


def assert_same_fields(got, want, what=""):
    for k, w in want.items():
        g = got[k]
        if w is None or g is None:
            assert w is None and g is None, f"{what}: {k} is {'NULL' if g is None else 'set'}"
        elif isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and np.array_equal(g, w), f"{what}: {k} differs"
        else:
            assert g == w, f"{what}: {k} differs"


def host_batch(text, clipping):
    """The host parser's batch of `text`, clipped at `clipping` (0: left as parsed)."""
    reads = snapgpu.Reads.from_fastq_bytes(text, name="case")
    if clipping:
        reads.clip(clipping)
    return reads


# ------------------------------------------------------------------ the texts
def rec(rid, bases, quals, plus=b"+", eol=b"\n"):
    return b"@" + rid + eol + bases + eol + plus + eol + quals + eol


def _q(front, mid, back):
    return b"#" * front + b"I" * mid + b"#" * back


_FOUR = b"".join(rec(b"r%d extra" % k, b"ACGTN"[k:] * (k + 9), b"5" * (len(b"ACGTN"[k:]) * (k + 9))) for k in range(4))
_B60 = b"ACGTACGTAC" * 6

CASES = {
    # empty and partial input
    "empty": b"",
    "three_lines": b"@a\nACGT\n+\n",
    "no_final_newline": b"@a\nACGT\n+\nIIII",
    "four_plus_1": _FOUR + b"@t",
    "four_plus_2": _FOUR + b"@t\nAC\n",
    "four_plus_3": _FOUR + b"@t\nAC\n+\n",
    # line endings and NUL bytes
    "crlf": rec(b"a", b"ACGT", b"IIII", eol=b"\r\n") + rec(b"b", b"GG", b"##", eol=b"\r\n"),
    "crcrlf": rec(b"a", b"ACGT", b"IIII", eol=b"\r\r\n") + rec(b"b x", b"GG", b"##", eol=b"\r\r\n"),
    "nul_in_id": rec(b"ab\0cd", b"ACGT", b"IIII") + rec(b"n", b"AC", b"II"),
    "nul_in_bases": rec(b"a", b"AC\0GT", b"IIIII") + rec(b"n", b"AC", b"II"),
    "nul_in_plus": rec(b"a", b"ACGT", b"IIII", plus=b"+\0x") + rec(b"n", b"AC", b"II"),
    "nul_in_quals": rec(b"a", b"ACGT", b"II\0I") + rec(b"n", b"AC", b"II"),
    "cr_before_nul": rec(b"a\r\0z", b"ACGT\r\0AA", b"IIII\r\0I"),
    "at_alone": rec(b"", b"ACGT", b"IIII") + rec(b"", b"", b""),
    # line lengths and contents
    "empty_bases": rec(b"a", b"", b"") + rec(b"b", b"", b"III") + rec(b"c", b"ACG", b"III"),
    "short_quals": rec(b"a", b"ACGTACGT", b"III") + rec(b"b", b"ACGT", b"") + rec(b"c", b"AC", b"II"),
    "long_quals": rec(b"a", b"ACG", b"IIIIIIII") + rec(b"b", b"AC", b"II"),
    "plus_repeats_id": rec(b"a b", b"ACGT", b"IIII", plus=b"+a b") + rec(b"c", b"AC", b"II", plus=b"+c"),
    "at_in_plus_and_quals": rec(b"a", b"ACGT", b"@III", plus=b"@a") + rec(b"b", b"AC", b"@@", plus=b"@"),
    "blank_lines_inside": b"@a\n\n\n\n@b\nAC\n+\nII\n",
    # clip edges (60 bases)
    "clip_all_hash": rec(b"a", _B60, b"#" * 60),
    "clip_leaves_49": rec(b"a", _B60, _q(5, 49, 6)) + rec(b"b", _B60, _q(11, 49, 0)) + rec(b"c", _B60, _q(0, 49, 11)),
    "clip_leaves_50": rec(b"a", _B60, _q(5, 50, 5)) + rec(b"b", _B60, _q(10, 50, 0)) + rec(b"c", _B60, _q(0, 50, 10)),
    "clip_front_only": rec(b"a", _B60, _q(7, 53, 0)),
    "clip_back_only": rec(b"a", _B60, _q(0, 52, 8)),
    "clip_short_quals": rec(b"a", _B60, _q(3, 52, 2)) + rec(b"b", _B60 + _B60, _q(4, 70, 3)),
    "clip_hash_inside": rec(b"a", _B60, b"##" + b"I" * 20 + b"#" * 5 + b"I" * 30 + b"###"),
}

BAD = {
    "bad_first": b"a\nACGT\n+\nIIII\n" + _FOUR,
    "bad_last": _FOUR + b"x@a\nACGT\n+\nIIII\n",
    "bad_nul_first_byte": _FOUR + b"\0@a\nACGT\n+\nIIII\n",
    "bad_empty_header": b"\nACGT\n+\nIIII\n",
    "bad_cr_only_header": _FOUR + b"\r\r\nACGT\n+\nIIII\n",
}
BAD_MESSAGE = "FASTQ record without '@' header in "


def _filler(nbytes, tag):
    """Whole records of 100 bases, `nbytes` bytes exactly (nbytes >= 12): the last one's id and body
    absorb the remainder."""
    out = []
    while nbytes >= 440:
        out.append(rec(b"%s%d" % (tag, len(out)), (b"ACGTTGCA" * 13)[:100], (b"IIII##5I" * 13)[:100]))
        nbytes -= len(out[-1])
    body = min(100, (nbytes - 8) // 2)            # "@" id "\n" body "\n+\n" body "\n" = 2 * body + 6 + id
    rid = tag + b"L" + b"p" * (nbytes - 2 * body - 8)
    out.append(rec(rid, (b"ACGTTGCA" * 13)[:body], (b"##III#5I" * 13)[:body]))
    assert len(out[-1]) == nbytes
    return b"".join(out)


def tile_cases(T):
    """Texts of exactly T-1, T, T+1 and 2T+1 bytes with a '\\n' as the last byte of a tile, one as the
    first byte of the next, a record across the tile edge -- and a text with one bases / quality line of
    T + 5000 bytes."""
    out = {}
    for size in (T - 1, T, T + 1, 2 * T + 1):
        for name, at in (("nl_last_of_tile", T - 1), ("nl_first_of_next", T), ("record_straddles", T + 40)):
            # a record boundary (its final '\n') at byte `at`, where the text is long enough
            if at >= size:
                at = size - 1
            head = _filler(at + 1, b"h")
            text = head + (_filler(size - len(head), b"t") if size - len(head) >= 12 else b"\n" * (size - len(head)))
            assert len(text) == size and text[at:at + 1] == b"\n"
            if text not in out.values():
                out[f"{name}_T{size - T:+d}" if size <= T + 1 else f"{name}_2T+1"] = text
    big = T + 5000
    out["long_line"] = (rec(b"first", b"ACGT" * 20, b"I" * 80) +
                        rec(b"long one", (b"ACGTTGCAAC" * (big // 10 + 1))[:big], b"###" + (b"IJKL5" * (big // 5 + 1))[:big - 7] + b"####") +
                        rec(b"after", b"GGCC" * 15, b"#" * 10 + b"I" * 50))
    out["long_line_short_quals"] = (rec(b"long two", b"A" * big, b"I" * (T // 2)) + rec(b"z", b"AC", b"II"))
    return out


def random_text(seed, n_records):
    """Seeded random records: lengths 0..300, ids 0..200 bytes, random '#' runs, mixed line endings."""
    rng = random.Random(seed)
    out = []
    for _ in range(n_records):
        n = rng.choice((0, 1, 49, 50, 51, 64, 100, 128, 150, 300, rng.randrange(301)))
        nid = rng.choice((0, 1, 20, 200, rng.randrange(201)))
        rid = bytes(rng.choice(b"abcXYZ019 /:_") for _ in range(nid))
        bases = bytes(rng.choice(b"ACGTN") for _ in range(n))
        f, b = rng.choice((0, 0, 1, 5, rng.randrange(n + 1))), rng.choice((0, 0, 1, 5, rng.randrange(n + 1)))
        q = bytearray(rng.choice(b"#5AIJ") for _ in range(n))
        q[:f] = b"#" * min(f, n)
        if b:
            q[n - min(b, n):] = b"#" * min(b, n)
        q = bytes(q)
        if rng.random() < 0.1:
            q = q[:rng.randrange(n + 1)]
        elif rng.random() < 0.1:
            q += b"I" * rng.randrange(9)
        if n and rng.random() < 0.03:
            k = rng.randrange(n)
            bases = bases[:k] + b"\0" + bases[k + 1:]
        eol = rng.choice((b"\n", b"\n", b"\n", b"\r\n", b"\r\r\n"))
        plus = rng.choice((b"+", b"+", b"+" + rid, b"@x"))
        out.append(rec(rid, bases, q, plus=plus, eol=eol))
    tail = rng.choice((b"", b"@t", b"@t\nAC\n", b"@t\nAC\n+"))
    return b"".join(out) + tail
