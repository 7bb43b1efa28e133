"""Helpers shared by test_bai_model.py (CPU) and test_bai_gpu.py; not a test.

Three independent things:
  expected_bai   a plain-Python restatement of the canonical .bai ("BAI on the device"):
                 dicts and lists, no code shared with csrc/bai_index.h
  parse_bai / query / brute_force
                 a reader that does what samtools does with an index: reg2bins, chunks cut by the
                 linear index's minimum offset, a seek by virtual offset with zlib on single members,
                 records read up to the chunk's end, an overlap filter
  make_records   raw BAM records packed with struct, and the fabricated streams built from them
"""
import struct
import zlib

MEMBER = 0xff00
PSEUDO_BIN = 37450
REF_OPS = (0, 2, 3, 7, 8)     # M D N = X consume the reference
M, I, D, N, S, EQ, X = 0, 1, 2, 3, 4, 7, 8


# ------------------------------------------------------------------ records
def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def reg2bins(beg, end):
    end -= 1
    bins = [0]
    for shift, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins.extend(range(base + (beg >> shift), base + (end >> shift) + 1))
    return bins


def _seq_len_for(body):
    """l_seq whose packed bases and qualities take exactly `body` bytes, or None."""
    if body % 3 == 0:
        return 2 * body // 3
    if body % 3 == 2:
        return 2 * (body - 2) // 3 + 1
    return None


def make_record(ref, pos, cigar=((50, M),), name_len=6, flag=0, l_seq=0, size=None, bin_=None):
    """One raw BAM record.  cigar: (length, op) pairs; name_len counts the NUL; size: the record's total
    bytes (block_size + 4), reached by choosing l_seq (and one more name byte if needed)."""
    if size is not None:
        l_seq = _seq_len_for(size - 36 - name_len - 4 * len(cigar))
        if l_seq is None:
            name_len += 1
            l_seq = _seq_len_for(size - 36 - name_len - 4 * len(cigar))
    span = max(1, sum(n for n, op in cigar if op in REF_OPS))
    if bin_ is None:
        bin_ = reg2bin(pos, pos + span) if ref >= 0 and pos >= 0 else 4680
    name = (b"r" * (name_len - 1)) + b"\0"
    body = struct.pack("<iiBBHHHiiii", ref, pos, name_len, 30, bin_, len(cigar), flag, l_seq, -1, -1, 0)
    body += name + b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar)
    body += bytes((7 * k + 1) & 0xff for k in range((l_seq + 1) // 2)) + bytes(30 + k % 11 for k in range(l_seq))
    rec = struct.pack("<i", len(body)) + body
    assert size is None or len(rec) == size, (len(rec), size)
    return rec


def make_records(specs):
    """specs: dicts of make_record's arguments -> the concatenated records."""
    return b"".join(make_record(**s) for s in specs)


def split(raw):
    out, at = [], 0
    while at < len(raw):
        bs = struct.unpack_from("<i", raw, at)[0]
        out.append(raw[at:at + 4 + bs])
        at += 4 + bs
    return out


def rec_fields(r):
    ref, pos, lrn, _, bin_, ncig, flag = struct.unpack_from("<iiBBHHH", r, 4)
    ops = struct.unpack_from("<%dI" % ncig, r, 36 + lrn)
    span = max(1, sum(v >> 4 for v in ops if (v & 15) in REF_OPS))
    return dict(ref=ref, pos=pos, bin=bin_, flag=flag, end=pos + span)


def fabricated():
    """name -> (records, n_ref): the streams test_bai_model.py lists, all in (refID, pos) order."""
    R = lambda ref, pos, **kw: dict(ref=ref, pos=pos, **kw)
    out = {}
    out["member_edges"] = (make_records([
        R(0, 100, size=30000), R(0, 200, size=MEMBER - 30000),          # ends exactly at byte 0xff00
        R(0, 20000, size=100),                                          # starts there, in another bin
        R(0, 20400, size=MEMBER), R(0, 40000, size=100),                # straddles byte 2 * 0xff00
        R(1, 5, size=MEMBER - 200), R(1, 20000)]), 2)                   # ends the third member, then another bin
    out["exactly_one_member"] = (make_records([R(0, 70000, size=MEMBER)]), 1)
    out["empty_reference_between"] = (make_records(
        [R(0, 10), R(0, 20000), R(2, 7), R(2, 8, flag=4), R(2, 40000)]), 4)
    out["window_3_only"] = (make_records([R(0, 3 * 16384 + 10), R(0, 3 * 16384 + 500), R(1, 3 * 16384 + 16000)]), 2)
    out["bins_not_contiguous"] = (make_records([
        R(0, 100), R(0, 200), R(0, 16350, cigar=((100, M),)),            # crosses 16 kb: level 4
        R(0, 16360, cigar=((10, M),)), R(0, 16370, cigar=((5, M),)),     # level 5 again: a second chunk of bin 4681
        R(0, 20000), R(0, 131000, cigar=((20, M),)),
        R(0, 131050, cigar=((100, M),)),                                 # crosses 128 kb: level 3
        R(0, 131060, cigar=((5, M),)), R(0, 140000)]), 1)
    out["long_N"] = (make_records([
        R(0, 1000, cigar=((10, M), (40000, N), (10, M))),                # windows 0, 1 and 2
        R(0, 1500), R(0, 20000), R(0, 20001, cigar=((30000, D),)), R(0, 60000), R(0, 200000)]), 1)
    out["span_1"] = (make_records([
        R(0, 16383, cigar=()), R(0, 16383, cigar=((50, S),)), R(0, 16383, cigar=((20, I), (30, S))),
        R(0, 5 * 16384 - 1, cigar=((40, S),)), R(0, 5 * 16384, cigar=())]), 1)
    out["only_unplaced"] = (make_records([R(-1, -1, flag=4, cigar=()) for _ in range(5)]), 2)
    out["equal_pos"] = (make_records([
        R(0, 16000, cigar=((10, M),)), R(0, 16000, cigar=((1000, M),)), R(0, 16000, cigar=((5, M),)),
        R(0, 16000, cigar=((40000, N), (1, M))), R(0, 17000), R(0, 17000, flag=4, cigar=()),
        R(1, 0, cigar=((1, M),)), R(-1, -1, flag=4, cigar=()), R(-1, 0, flag=4, cigar=())]), 3)
    return out


# ------------------------------------------------------------------ the restatement
def members_of(bgzf):
    """[(compressed start, compressed size, ISIZE)] of a BGZF stream with the standard 18-byte header."""
    out, at = [], 0
    while at < len(bgzf):
        assert bgzf[at:at + 4] == b"\x1f\x8b\x08\x04" and bgzf[at + 12:at + 14] == b"BC"
        size = struct.unpack_from("<H", bgzf, at + 16)[0] + 1
        out.append((at, size, struct.unpack_from("<I", bgzf, at + size - 4)[0]))
        at += size
    return out


def expected_bai(records, bgzf, n_ref, stream_offset=0):
    members = members_of(bgzf)
    assert sum(m[2] for m in members) == len(records)
    data_end = len(bgzf)
    for at, _, isize in reversed(members):     # where the members that hold nothing (the EOF block) begin
        if isize:
            break
        data_end = at

    def voff(u):
        before = 0
        for at, _, isize in members:
            if u < before + isize:
                return (stream_offset + at) << 16 | (u - before)
            before += isize
        return (stream_offset + data_end) << 16

    refs = [dict(bins={}, lin={}, mapped=0, unmapped=0, first=None, last=None) for _ in range(n_ref)]
    no_coor, u, prev = 0, 0, None
    for r in split(records):
        f = rec_fields(r)
        beg_v, end_v = voff(u), voff(u + len(r))
        u += len(r)
        if f["ref"] < 0:
            no_coor += 1
            prev = None
            continue
        ref = refs[f["ref"]]
        chunks = ref["bins"].setdefault(f["bin"], [])
        if prev == (f["ref"], f["bin"]):
            chunks[-1][1] = end_v
        else:
            chunks.append([beg_v, end_v])
        prev = (f["ref"], f["bin"])
        if ref["first"] is None:
            ref["first"] = beg_v
        ref["last"] = end_v
        ref["unmapped" if f["flag"] & 4 else "mapped"] += 1
        for w in range(f["pos"] >> 14, ((f["end"] - 1) >> 14) + 1):
            ref["lin"][w] = min(ref["lin"].get(w, beg_v), beg_v)
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for ref in refs:
        if ref["first"] is None:
            out.append(struct.pack("<ii", 0, 0))
            continue
        out.append(struct.pack("<i", len(ref["bins"]) + 1))
        for b in sorted(ref["bins"]):
            out.append(struct.pack("<Ii", b, len(ref["bins"][b])))
            out.extend(struct.pack("<QQ", *c) for c in ref["bins"][b])
        out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, ref["first"], ref["last"], ref["mapped"], ref["unmapped"]))
        n_intv = max(ref["lin"]) + 1
        lin, above = [0] * n_intv, None
        for w in range(n_intv - 1, -1, -1):
            above = ref["lin"].get(w, above)
            lin[w] = above
        out.append(struct.pack("<i", n_intv) + struct.pack("<%dQ" % n_intv, *lin))
    out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


# ------------------------------------------------------------------ the reader
def parse_bai(bai):
    assert bai[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<i", bai, 4)[0]
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", bai, at)[0]
        at += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", bai, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            if b == PSEUDO_BIN:
                meta = chunks
            else:
                assert b not in bins and b < PSEUDO_BIN
                bins[b] = chunks
        n_intv = struct.unpack_from("<i", bai, at)[0]
        lin = list(struct.unpack_from("<%dQ" % n_intv, bai, at + 4))
        at += 4 + 8 * n_intv
        refs.append(dict(bins=bins, meta=meta, lin=lin))
    no_coor = struct.unpack_from("<Q", bai, at)[0]
    assert at + 8 == len(bai)
    return dict(refs=refs, no_coor=no_coor)


class _Cursor:
    """Sequential reads of the uncompressed data of a BGZF file from a virtual offset on."""

    def __init__(self, file_bytes, v):
        self.f = file_bytes
        self._load(v >> 16)
        self.o = v & 0xffff

    def _load(self, coff):
        self.c = coff
        self.size = struct.unpack_from("<H", self.f, coff + 16)[0] + 1
        self.data = zlib.decompress(self.f[coff:coff + self.size], 31)

    def tell(self):
        while self.o == len(self.data) and self.c + self.size < len(self.f):   # the end of a member is the start of the next
            self._load(self.c + self.size)
            self.o = 0
        return self.c << 16 | self.o

    def read(self, n):
        out = b""
        while len(out) < n:
            self.tell()
            take = self.data[self.o:self.o + n - len(out)]
            assert take, "read past the end of the file"
            out += take
            self.o += len(take)
        return out


def query(file_bytes, bai, ref, beg, end):
    """The records of reference `ref` that overlap [beg, end), found through the index as samtools does."""
    idx = parse_bai(bai)["refs"][ref]
    if not idx["lin"]:
        return []
    w = beg >> 14
    min_off = idx["lin"][w] if w < len(idx["lin"]) else idx["lin"][-1]
    chunks = sorted(c for b in reg2bins(beg, end) for c in idx["bins"].get(b, ()) if c[1] > min_off)
    out, seen = [], set()
    for c_beg, c_end in chunks:
        cur = _Cursor(file_bytes, c_beg)
        while cur.tell() < c_end:
            at = cur.tell()
            head = cur.read(4)
            r = head + cur.read(struct.unpack("<i", head)[0])
            f = rec_fields(r)
            if f["ref"] != ref or f["pos"] >= end:
                break
            if f["end"] > beg and at not in seen:
                seen.add(at)
                out.append(r)
    return out


def brute_force(records, ref, beg, end):
    return [r for r in split(records) for f in [rec_fields(r)] if f["ref"] == ref and f["pos"] < end and f["end"] > beg]
