"""Helpers shared by test_dupmark_model.py (CPU) and test_dupmark_gpu.py; not a test.

  expected_marks  a plain-Python restatement of the marking rule ("Duplicate marking on the
                  device") over bai_cases.split: dicts and tuples, no code shared with csrc/dupmark_rule.h
  rec / stream    raw single-end BAM records with chosen qualities, over bai_cases.make_record
  fabricated      the streams the two test files run, a few KB each; refusals() the refused ones

The device passes work in tiles of 32 records (the score pass: 256 threads, 8 lanes per record), 64 lanes
(a wave) and 256 records (the best, mark and check passes); "tile_edges" holds a group across each boundary.
"""
import random
import struct

from bai_cases import make_record, split

DUP, UNMAPPED, REVERSE, MATE = 0x400, 0x4, 0x10, 0x1
TILES = (32, 64, 256)
EINVAL, EFORMAT = -1, -5


# ------------------------------------------------------------------ the restatement
def qual_of(r):
    lrn, ncig, l_seq = r[12], struct.unpack_from("<H", r, 16)[0], struct.unpack_from("<i", r, 20)[0]
    at = 36 + lrn + 4 * ncig + (l_seq + 1) // 2
    return r[at:at + l_seq]


def expected_marks(raw, n_ref):
    """-> (the records with 0x400 as the rule sets it, n_marked, n_groups of two or more)."""
    recs = split(raw)
    groups = {}
    for i, r in enumerate(recs):
        ref, pos = struct.unpack_from("<ii", r, 4)
        flag = struct.unpack_from("<H", r, 18)[0]
        if 0 <= ref < n_ref and pos >= 0 and not flag & UNMAPPED:
            score = sum(q for q in qual_of(r) if q != 0xff)
            groups.setdefault((ref, pos, flag & REVERSE), []).append((score, -i))
    marked = set()
    for members in groups.values():
        kept = max(members)                   # the highest score, the earliest among equals
        marked.update(-m[1] for m in members if m != kept)
    out = []
    for i, r in enumerate(recs):
        flag = struct.unpack_from("<H", r, 18)[0]
        flag = flag | DUP if i in marked else flag & ~DUP
        out.append(r[:18] + struct.pack("<H", flag) + r[20:])
    return b"".join(out), len(marked), sum(len(m) >= 2 for m in groups.values())


def only_byte_19_differs(before, after):
    a, b = split(before), split(after)
    return len(before) == len(after) and len(a) == len(b) and all(
        x[:19] == y[:19] and x[20:] == y[20:] and (x[19] ^ y[19]) & ~0x04 == 0 for x, y in zip(a, b))


def without_marks(raw):
    return b"".join(r[:19] + bytes([r[19] & ~0x04]) + r[20:] for r in split(raw))


# ------------------------------------------------------------------ records
def rec(ref, pos, quals=(30,) * 20, flag=0, name_len=6):
    """One record whose QUAL bytes are `quals`."""
    quals = bytes(quals)
    r = make_record(ref, pos, cigar=((max(1, len(quals)), 0),), name_len=name_len, flag=flag, l_seq=len(quals))
    return r[:len(r) - len(quals)] + quals


def _quals(rng, n, lo=2, hi=41):
    return bytes(rng.randrange(lo, hi) for _ in range(n))


def _group(rng, ref, pos, n, l_seq=20, flag=0):
    return [rec(ref, pos, _quals(rng, l_seq), flag=flag) for _ in range(n)]


def fabricated():
    """name -> (records, n_ref), all in (refID, pos) order."""
    rng = random.Random(20)
    unplaced = lambda flag=UNMAPPED: rec(-1, -1, _quals(rng, 12), flag=flag)
    out = {}
    out["no_records"] = (b"", 3)
    out["one_record"] = (rec(0, 100, _quals(rng, 50)), 3)
    out["unmapped_only"] = (b"".join(unplaced(f) for f in (4, 4 | DUP, 4, 4 | REVERSE, 4 | DUP)), 3)
    out["two_equal_scores"] = (rec(1, 7, (30,) * 40) + rec(1, 7, (30,) * 40), 3)
    out["strands_alternate"] = (b"".join(
        rec(0, 500, _quals(rng, 30), flag=REVERSE if k % 2 else 0) for k in range(5)), 3)
    out["same_pos_two_references"] = (rec(0, 100, _quals(rng, 25)) + rec(1, 100, _quals(rng, 25)) +
                                      rec(1, 100, _quals(rng, 25)) + rec(2, 100, _quals(rng, 25)), 3)
    out["group_of_65"] = (b"".join([rec(0, 5)] + _group(rng, 0, 900, 65) + [rec(0, 901)]), 3)
    big = _group(rng, 1, 4000, 2049, l_seq=8)
    big[1500] = rec(1, 4000, (41,) * 8)                  # the one kept, deep inside
    out["group_of_2049"] = (b"".join([rec(0, 1), rec(0, 1, flag=REVERSE)] + big + [rec(2, 0)]), 3)
    out["best_is_last"] = (b"".join(_group(rng, 0, 10, 6, l_seq=33) + [rec(0, 10, (41,) * 33)]), 3)
    # groups of 4 across records 32, 64 and 256 (and 2 * 32 = 64 in the group numbering), singletons between
    recs, pos = [], 0
    while len(recs) < 300:
        pos += 3
        if len(recs) + 2 in TILES:
            recs += [rec(0, pos, _quals(rng, 21), flag=REVERSE if k == 1 else 0) for k in range(4)]
        else:
            recs.append(rec(0, pos, _quals(rng, 21)))
    out["tile_edges"] = (b"".join(recs), 3)
    out["sequence_lengths"] = (b"".join(
        [rec(0, 10, ()), rec(0, 10, ()), rec(0, 20, (7,)), rec(0, 20, (9,)), rec(0, 20, (9,))] +
        _group(rng, 0, 30, 3, l_seq=1024) + [rec(0, 30, (254,) * 1024), rec(0, 40, (0xff,) * 1024)]), 3)
    out["quals_all_missing"] = (b"".join(rec(2, 77, (0xff,) * n) for n in (5, 40, 41, 3)), 3)
    out["scores_all_zero"] = (b"".join([rec(2, 5, (0,) * 30), rec(2, 5, (0xff,) * 30), rec(2, 5, (0, 0xff) * 15)]), 3)
    out["name_lengths"] = (b"".join(
        rec(1, 100 * k, _quals(rng, 17 + (k + j) % 9), name_len=k) for k in range(1, 17) for j in range(4)), 3)
    out["stray_marks"] = (b"".join([
        rec(0, 9, (40,) * 20, flag=DUP), rec(0, 9, (20,) * 20),            # on the kept one; the other lacks it
        rec(0, 9, (39,) * 20, flag=UNMAPPED | DUP),                        # placed, unmapped: no member of the group
        rec(0, 9, (30,) * 20, flag=DUP), rec(0, 12, (30,) * 20, flag=DUP | REVERSE),
        unplaced(UNMAPPED | DUP), unplaced()]), 3)
    out["unmapped_inside_a_group"] = (b"".join([
        rec(0, 50, (10,) * 20), rec(0, 50, (41,) * 20, flag=UNMAPPED), rec(0, 50, (12,) * 20),
        rec(0, 50, (11,) * 20, flag=REVERSE), rec(0, 50, (12,) * 20)]), 3)
    out["ends_in_a_group"] = (b"".join([rec(0, 1)] + _group(rng, 2, 800, 5)), 3)
    out["ends_in_unmapped"] = (b"".join(_group(rng, 2, 800, 5) + [unplaced(), unplaced(4 | DUP)]), 3)
    return out


def refusals():
    """name -> (records, n_ref, the model's code)."""
    good = [rec(0, 10), rec(0, 10), rec(1, 5), rec(-1, -1, flag=UNMAPPED)]
    long_seq = bytearray(rec(0, 10))
    long_seq[20:24] = struct.pack("<i", (1 << 24) + 1)
    short_qual = bytearray(rec(0, 10, (30,) * 20))
    short_qual[20:24] = struct.pack("<i", 24)             # its QUAL passes its end
    return {
        "mate": (b"".join([good[0], rec(0, 10, flag=MATE | 0x40)] + good[2:]), 2, EINVAL),
        "out_of_order": (b"".join([good[0], good[2], good[1], good[3]]), 2, EFORMAT),
        "position_goes_down": (b"".join([good[0], rec(0, 9)] + good[2:]), 2, EFORMAT),
        "truncated": (b"".join(good)[:-3], 2, EFORMAT),
        "truncated_header": (b"".join(good[:2]) + good[2][:20], 2, EFORMAT),
        "refid_is_nref": (b"".join(good[:3] + [rec(2, 5), good[3]]), 2, EFORMAT),
        "negative_pos": (b"".join(good[:2] + [rec(1, -1)] + good[2:]), 2, EFORMAT),
        "l_seq_above_2_24": (bytes(long_seq) + b"".join(good), 2, EFORMAT),
        "qual_passes_the_end": (bytes(short_qual) + b"".join(good), 2, EFORMAT),
    }


def random_stream(rng, n_records, n_ref=3):
    """Up to n_records records over few distinct positions, so that groups form; sorted."""
    keys = []
    for _ in range(n_records):
        if rng.random() < 0.1:
            keys.append((n_ref, 0))
        else:
            keys.append((rng.randrange(n_ref), rng.randrange(1 + n_records // 6)))
    out = []
    for ref, pos in sorted(keys):
        flag = (REVERSE if rng.random() < 0.4 else 0) | (DUP if rng.random() < 0.2 else 0)
        if ref == n_ref:
            out.append(rec(-1, -1, _quals(rng, rng.randrange(0, 30)), flag=flag | UNMAPPED, name_len=rng.randrange(1, 20)))
            continue
        if rng.random() < 0.1:
            flag |= UNMAPPED
        lo, hi = rng.choice([(2, 41), (30, 32), (0, 1), (250, 256)])
        out.append(rec(ref, pos, _quals(rng, rng.randrange(0, 60), lo, hi), flag=flag, name_len=rng.randrange(1, 20)))
    return b"".join(out)
