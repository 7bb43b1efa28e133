"""Deterministic cases for the two LV unit kernels (tests/test_lv_pass.py, tests/test_lv_filter.py).

Part A, scoring passes (snapgpu.lv_pass_batch): pass_cases(GS, NW) lists passes of one read each whose lane
groups hold different candidates; expected_pass() scores a pass with the oracle's LandauVishkin
(oracle/snap_oracle.c oracle_lv, pinned to the reference's vectors by test_oracle_golden.py) called as
BaseAligner::score calls it.  Part B, the forced-mode prefilter (snapgpu.lv_filter_batch): filter_genome() and
filter_tasks() make a two-contig genome and tasks over it; expected_filter() gives the encoded word.

Every candidate is made from its read: the genome bytes around it are the read's, with a recipe's edits applied
to the side after the seed (the forward call's text) and to the side before it (the reverse call's text, walked
backwards), random bytes beyond.  A recipe states an intent; what a case exercises is decided by the oracle
(coverage(), the tests' own counts), never by the code under test.
"""
import random

from oracle_ffi import oracle_lv_at

MAX_K = 31
KS = (0, 1, 3, 4, 7, 8, 15, 16, 30)                      # both edges of every group size's range
NS = {2: (17, 63, 64, 65, 127, 128), 4: (129, 191, 192, 193, 255, 256)}
SEED_LENS = (16, 20)
ACGT = b"ACGT"
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
GUARD = MAX_K + 9                                         # genome bytes kept beyond what a call may look at


def group_size(k):
    k = min(k, MAX_K - 1)
    return 8 if k <= 3 else 16 if k <= 7 else 32 if k <= 15 else 64


def revcomp(b):
    return b.translate(_COMP)[::-1]


def _rand_bases(rng, n):
    return bytes(rng.choice(ACGT) for _ in range(n))


def _other(rng, c):
    return rng.choice([x for x in ACGT if x != c])


def _edit(rng, pat, ops):
    """The text a pattern aligns to under ops {position: (kind, length)}: 'sub' the text base differs, 'subn' it
    is an 'n', 'ins' the text holds `length` extra bases before the position, 'del' it lacks `length` pattern
    bases."""
    out = bytearray()
    i = 0
    while i < len(pat):
        kind, ln = ops.get(i, (None, 0))
        if kind == "sub":
            out.append(_other(rng, pat[i])); i += 1
        elif kind == "subn":
            out.append(ord("n")); i += 1
        elif kind == "ins":
            out.append(_other(rng, pat[i])); out += _rand_bases(rng, ln - 1)
            out.append(pat[i]); i += 1
        elif kind == "del":
            i += ln
        else:
            out.append(pat[i]); i += 1
    return bytes(out)


def _side_ops(rng, L, spec):
    """Edit positions on a side of L pattern bases for spec {sub: count, indel: (kind, run, adjacent_sub), last,
    dense}.  Returns (ops, edits, net indel, whether the side could hold them)."""
    nsub, indel, last = spec.get("sub", 0), spec.get("indel"), spec.get("last", False)
    ops, used = {}, set()
    edits = net = 0
    if indel:
        kind, run, adj = indel
        need = run + 2 + (1 if adj else 0)
        if L < need + 1:
            return {}, 0, 0, False
        p = rng.randrange(1, L - need + 1)
        ops[p] = (kind, run)
        span = run if kind == "del" else 1
        for q in range(p - 1, p + span + 1):
            used.add(q)
        if adj:   # a substitution with no matched base between it and the run
            q = p + span if kind == "del" else p + 1
            ops[q] = ("sub", 1)
            used.update((q, q + 1))
            edits += 1
        edits += run
        net = run if kind == "del" else -run
    if last and L >= 1 and (L - 1) not in used:
        ops[L - 1] = ("sub", 1)
        used.update((L - 1, L - 2))
        edits += 1
        nsub -= 1
    free = [q for q in range(L) if q not in used]
    if nsub > len(free):
        return {}, 0, 0, False
    # spaced substitutions where the side is long enough, any distinct positions otherwise
    spaced = [q for q in free if q % 2 == 0]
    pool = spaced if nsub <= len(spaced) and not spec.get("dense") else free
    for q in rng.sample(pool, max(0, nsub)):
        ops[q] = ("subn", 1) if rng.random() < 0.08 else ("sub", 1)
        edits += 1
    return ops, edits, net, True


def make_candidate(rng, read, n, seed_len, recipe):
    """One candidate of a pass from its recipe -> the dict lv_pass_batch takes, plus the recipe."""
    d = rng.randrange(2)
    rd = revcomp(read) if d else read
    fs, rs = recipe.get("f", {}), recipe.get("r", {})
    need_f = fs.get("sub", 0) + (fs["indel"][1] + 4 if fs.get("indel") else 0)
    need_r = rs.get("sub", 0) + (rs["indel"][1] + 4 if rs.get("indel") else 0)
    smax = n - seed_len
    opts = [s for s in (0, 1, smax, smax // 2, smax // 3, (2 * smax) // 3, rng.randrange(smax + 1))
            if s >= need_r and smax - s >= need_f]
    if need_f + need_r >= 16 and (need_f == 0 or need_r == 0):   # many edits on one side: make it the long one
        s = smax - rng.randrange(2) if need_f == 0 else rng.randrange(2)
    elif opts:
        s = rng.choice(opts)
    else:
        s = min(smax, max(need_r, smax * need_r // max(1, need_f + need_r)))
    t = s + seed_len
    pf, pr = rd[t:], rd[:s][::-1]
    of, ef, nf, okf = _side_ops(rng, len(pf), fs)
    orv, er, nr, okr = _side_ops(rng, len(pr), rs)
    if recipe.get("random"):
        tf, tr = _rand_bases(rng, len(pf)), _rand_bases(rng, len(pr))
    else:
        tf, tr = _edit(rng, pf, of), _edit(rng, pr, orv)
    tf += _rand_bases(rng, 2 * MAX_K + GUARD)
    tr += _rand_bases(rng, 2 * MAX_K + GUARD)
    genome = (tr[::-1] + rd[s:t] + tf).replace(b"N", b"n")   # a genome's N is 'n': it matches no read base
    glen = n + MAX_K
    if recipe.get("short_glen"):   # the contig-end fallback's window, real bytes past it
        lo = max(t, n - MAX_K)
        glen = rng.randrange(lo, n + MAX_K)
    return dict(genome=genome, before=len(tr) - s, dir=d, s=s, act=0 if recipe.get("inactive") else 1, glen=glen,
                recipe=recipe, intent=dict(ef=ef, er=er, nf=nf, nr=nr, ok=okf and okr))


def _recipes(k, GS):
    """The candidate recipes of limit k: every distance on each side, the named kinds, failures."""
    R = []
    for dd in range(0, k + 1):
        for _ in range(2 if dd >= 20 else 1):   # dense substitutions often align cheaper than their count
            R.append(dict(kind="fwd", f=dict(sub=dd)))
            R.append(dict(kind="rev", r=dict(sub=dd)))
        R.append(dict(kind="at_k", f=dict(sub=dd), r=dict(sub=k - dd)))          # succeeds at exactly k
    R.append(dict(kind="e1_is_k", f=dict(sub=k)))                                  # k2 = 0
    R.append(dict(kind="e2_is_k", r=dict(sub=k)))
    R.append(dict(kind="exact"))
    R.append(dict(kind="exact", short_glen=True))
    R.append(dict(kind="inactive", inactive=True))
    R.append(dict(kind="fail", f=dict(sub=k + 1)))
    R.append(dict(kind="fail", r=dict(sub=k + 1)))
    R.append(dict(kind="fail", f=dict(sub=k // 2 + 1), r=dict(sub=k - k // 2)))    # k + 1 over both sides
    R.append(dict(kind="fail", random=True))
    R.append(dict(kind="fail", f=dict(sub=k + 2)))
    R.append(dict(kind="fail", r=dict(sub=k + 2)))
    R.append(dict(kind="fail", f=dict(sub=1), r=dict(sub=k)))
    if k >= 1:
        R.append(dict(kind="last", f=dict(sub=1, last=True)))                      # substitution at the last pattern base
        R.append(dict(kind="last", r=dict(sub=1, last=True)))
        R.append(dict(kind="dense", f=dict(sub=min(k, 3), dense=True)))
        R.append(dict(kind="short", f=dict(sub=min(k, 2)), short_glen=True))
    for side in ("f", "r"):
        for ik in ("ins", "del"):
            for run in (1, 2, 3, 4):
                if run <= k:
                    R.append({"kind": f"run{min(run, 3)}", side: dict(indel=(ik, run, False))})
                    if run + 1 <= k:
                        R.append({"kind": "adj", side: dict(indel=(ik, run, True))})
                    if run + 2 <= k:
                        R.append({"kind": f"run{min(run, 3)}", side: dict(indel=(ik, run, False), sub=2)})
            if k >= 5:   # a run as long as the path allows, next to the diagonal band's edge
                R.append({"kind": "run3", side: dict(indel=(ik, min(k, GS // 2 - 1) - 1, False))})
    return R


def pass_cases(GS, NW, reps=None):
    """Passes for lv_pass_batch at group size GS on NW mask words: every k of KS that chooses GS, every n of
    NS[NW], seed lengths 16 and 20, full passes and passes with 1 and Gn - 1 candidates; the recipes of a k are
    dealt round the groups so that the groups of a pass differ and every kind lands in every group."""
    rng = random.Random(7919 * GS + NW)
    Gn = 64 // GS
    reps = reps or {8: 3, 16: 3, 32: 11, 64: 14}[GS]
    passes = []
    for k in (k for k in KS if group_size(k) == GS):
        R = _recipes(k, GS)
        deck = []
        for r in range(reps * Gn):
            rot = R[r % len(R):] + R[:r % len(R)]
            deck += rot if r % 2 == 0 else rot[::-1]
        pos = pi = 0
        while pos < len(deck):
            fill = (Gn, Gn, 1, max(1, Gn - 1))[pi % 4]
            n = NS[NW][pi % len(NS[NW])]
            seed_len = SEED_LENS[(pi // len(NS[NW])) % 2]
            if n < seed_len:
                seed_len = 16
            chunk = deck[pos:pos + fill]
            pos += fill
            need = max(sum(rc.get(sd, {}).get("sub", 0) for sd in "fr") for rc in chunk)
            if n > NS[NW][0] and (need >= 16 or n - seed_len < need + 2):   # the sides must hold the edits: the two longest reads
                n = NS[NW][-1 - pi % 2]
            read = bytearray(_rand_bases(rng, n))
            if pi % 11 == 5:
                read[rng.randrange(n)] = ord("N")
            read = bytes(read)
            quals = bytes(rng.randrange(ord("!"), ord("M") + 1) for _ in range(n))
            # (a deck ordered by the rotation would put recipe j into group j % Gn every time: shift per pass)
            shift = pi % Gn
            chunk = chunk[shift % len(chunk):] + chunk[:shift % len(chunk)]
            cands = [make_candidate(rng, read, n, seed_len, rc) for rc in chunk]
            passes.append(dict(read=read, quals=quals, seedLen=seed_len, k=k, cands=cands))
            pi += 1
    return passes


def expected_pass(p):
    """The oracle's result per candidate of a pass: (e1, e2, p1, p2, net2) with e2 = -1 when the reverse call is
    not reached (an inactive candidate: e1 = e2 = -1)."""
    n, k, sl = len(p["read"]), p["k"], p["seedLen"]
    out = []
    for c in p["cands"]:
        if c is None or not c["act"]:
            out.append((-1, -1, 1.0, 1.0, 0))
            continue
        rd = revcomp(p["read"]) if c["dir"] else p["read"]
        qd = p["quals"][::-1] if c["dir"] else p["quals"]
        s, t = c["s"], c["s"] + sl
        e1, _, p1 = oracle_lv_at(1, c["genome"], c["before"] + t, c["glen"] - t, rd[t:], qd[t:], k)
        e2, net, p2 = -1, 0, 1.0
        if e1 >= 0:
            e2, net, p2 = oracle_lv_at(-1, c["genome"], c["before"] + s, c.get("rtl", s + MAX_K), rd[:s][::-1],
                                       qd[:s][::-1], k - e1)
        out.append((e1, e2, p1, p2, net))
    return out


INDEL_KINDS = ("run1", "run2", "run3", "adj")


def coverage(passes, expected):
    """What the oracle says the passes exercise, per LV direction ('f', 'r'):
    dist[dir][d] successes of that call at distance d, fail[dir] failed calls, group[dir][gi] successful calls
    in lane group gi, kinds[dir][kind] successful calls whose recipe put that indel pattern on that side and
    whose oracle distance and netIndel are the recipe's (so the path holds exactly that run)."""
    cov = {d: dict(dist={}, fail=0, group={}, kinds={}) for d in "fr"}
    for p, exp in zip(passes, expected):
        for gi, (c, (e1, e2, _, _, net2)) in enumerate(zip(p["cands"], exp)):
            if c is None or not c["act"]:
                continue
            calls = [("f", e1, True)] + ([("r", e2, True)] if e1 >= 0 else [])
            for d, e, _ in calls:
                v = cov[d]
                if e < 0:
                    v["fail"] += 1
                    continue
                v["dist"][e] = v["dist"].get(e, 0) + 1
                v["group"][gi] = v["group"].get(gi, 0) + 1
                spec = c["recipe"].get(d, {})
                it = c["intent"]
                kind = c["recipe"]["kind"]
                if kind in INDEL_KINDS and spec.get("indel") and it["ok"]:
                    want_e = it["ef"] if d == "f" else it["er"]
                    if e == want_e and (d == "f" or net2 == it["nr"]):
                        v["kinds"][kind] = v["kinds"].get(kind, 0) + 1
    return cov


# ---------------------------------------------------------------------------------- part B: the prefilter
FKM, LQ_K, NPAD = 5, 7, 100
FRES_VALID = 1 << 31
FILTER_SEED_LEN = 20
FILTER_PADDING = 500


def filter_genome():
    """Two contigs of about 10 kb, as (name, sequence) for a FASTA file; a short 'N' run inside the first."""
    rng = random.Random(424242)
    a = bytearray(_rand_bases(rng, 10_007))
    a[5000:5003] = b"NNN"
    b = _rand_bases(rng, 9_981)
    return [("chrA", bytes(a).decode()), ("chrB", b.decode())]


def _servable(pieces, n_bases, padding, offset, length):
    """Genome::getSubstring != NULL (Genome.h:78-148).  A window no longer than the padding is always served; with
    at most 100 contigs so is every window that starts at or after the first contig (sic), so only a genome of
    more than 100 contigs with a padding shorter than the window has windows that a contig end leaves unserved."""
    if offset > n_bases or offset + length > n_bases + NPAD:
        return False
    if length <= padding:
        return True
    if len(pieces) > 100:
        if pieces[-1] <= offset:
            return True
        lo, hi = 0, len(pieces) - 2
        while lo <= hi:
            m = (lo + hi) // 2
            if pieces[m] <= offset:
                if pieces[m + 1] > offset:
                    return not pieces[m + 1] <= offset + length - 1
                lo = m + 1
            else:
                hi = m - 1
        return False
    for po in pieces:
        if offset + length - 1 >= po:
            return not offset < po
    return False


MANY_PADDING = 40


def filter_genome_many():
    """130 contigs of 200 bases: with MANY_PADDING between them, a window of n + MAX_K bases that reaches the next
    contig's start is not servable (Genome.h:98-134, the search over more than 100 contigs)."""
    rng = random.Random(515151)
    return [(f"c{i}", _rand_bases(rng, 200).decode()) for i in range(130)]


def filter_edge_tasks(quad, bases, pieces, n_bases):
    """Tasks over filter_genome_many(): windows that end exactly at the next contig's start, up to three bases short
    of it (they hold the padding's 'n's) and up to three past it, and windows inside the contig; reads cut from the
    genome there (some with a substitution).  A window that reaches the next contig is not settled by the prefilter
    and must give 0."""
    rng = random.Random(77 + (1 if quad else 0))
    KM = LQ_K if quad else FKM
    T = []
    n = 100
    for i in range(3, len(pieces) - 1, 5):
        end = pieces[i + 1]
        for off in (-MANY_PADDING - 4, -MANY_PADDING - 1, -MANY_PADDING) + tuple(range(-3, 4)):
            loc = end - (n + MAX_K) + off
            s = rng.randrange(0, n - FILTER_SEED_LEN + 1)
            T.append((_read_at(rng, bases, loc, n, s, FILTER_SEED_LEN, off & 1, ("sub", i % 3), (None, 0)), loc, off & 1, s,
                      rng.randrange(0, KM + 1), 1))
    return T


def _read_at(rng, bases, loc, n, s, seed_len, d, fside, rside):
    """A read[dir] of n bases whose seed [s, s + seed_len) sits at loc + s of the genome bytes `bases`, the sides
    made by undoing edits: side spec (kind, count) with kind 'sub', 'del' (count genome bases are missing from
    the read: the forward path ends on diagonal +count), 'ins' (count extra read bases: diagonal -count), or a
    list of such specs."""
    def side(L, text_at, spec):
        # read side of L bases against the genome text text_at(j), j = 0.. (walked in LV order)
        out = bytearray()
        j = 0
        specs = spec if isinstance(spec, list) else [spec]
        marks = {}
        for kind, cnt in specs:
            if not kind or cnt <= 0 or L < cnt + 4:
                continue
            if kind == "sub":
                for q in rng.sample(range(0, L), min(cnt, L)):
                    marks[q] = ("sub", 1)
            else:
                marks[rng.randrange(2, L - cnt - 1)] = (kind, cnt)
        while len(out) < L:
            kind, cnt = marks.get(len(out), (None, 0))
            if kind == "sub":
                out.append(_other(rng, text_at(j))); j += 1
            elif kind == "del":
                marks.pop(len(out))
                j += cnt
            elif kind == "ins":
                marks.pop(len(out))
                out += bytes(_other(rng, text_at(j)) for _ in range(1)) + _rand_bases(rng, cnt - 1)
            else:
                out.append(text_at(j)); j += 1
        return bytes(out[:L])

    up = lambda c: c - 32 if 97 <= c <= 122 else c
    t = s + seed_len
    fwd = side(n - t, lambda j: up(bases[loc + t + j]), fside)
    rev = side(s, lambda j: up(bases[loc + s - 1 - j]), rside)
    rd = rev[::-1] + bytes(up(c) for c in bases[loc + s:loc + t]) + fwd
    rd = bytes(c if c in ACGT else ord("N") for c in rd)
    return revcomp(rd) if d else rd   # the forward read the aligner is given


def filter_tasks(quad, bases, pieces, n_bases):
    """Tasks (read, loc, dir, s, k, act) for lv_filter_batch in the pair (k <= 5) or quad (k <= 7) form over the
    genome bytes `bases` with contig starts `pieces`.  Within a wave neighbouring tasks alternate between
    active, inactive, exact match and failures; the last wave holds a single task."""
    rng = random.Random(99 + (1 if quad else 0))
    KM = LQ_K if quad else FKM
    c0, c1 = pieces[0], pieces[1]
    end0 = c1 - FILTER_PADDING          # first contig's end (padding follows)
    sl = FILTER_SEED_LEN
    T = []

    def add(loc, n, s, d, k, fside=(None, 0), rside=(None, 0), act=1):
        T.append((_read_at(rng, bases, loc, n, s, sl, d, fside, rside), loc, d, s, k, act))

    def interior(n):
        while True:
            loc = rng.randrange(c0 + 40, end0 - n - 80)
            if not 4960 + c0 - n - 40 < loc < 5010 + c0:   # keep clear of the N run
                return loc

    # every word phase of the plane window, exact and lightly edited
    base = interior(128)
    for ph in range(32):
        n = rng.choice((101, 128, 76))
        add(base + ph, n, rng.randrange(0, n - sl + 1), ph & 1, rng.randrange(0, KM + 1), ("sub", rng.randrange(0, 3)))
    # indels of every size on either side of the seed, both signs, both directions, at limits d and d - 1
    for d in range(1, KM + 1):
        for kind in ("del", "ins"):
            for rc in (0, 1):
                for side in ("f", "r"):
                    for rep in range(12):
                        n = rng.choice((100, 101, 120, 128))
                        s = rng.randrange(0, 6) if side == "f" else n - sl - rng.randrange(0, 6)
                        loc = interior(n)
                        fs, rs = ((kind, d), (None, 0)) if side == "f" else ((None, 0), (kind, d))
                        add(loc, n, s, rc, d, fs, rs)
                        add(loc, n, s, rc, d - 1, fs, rs)
    # mixed substitutions and indels at every limit
    for k in range(0, KM + 1):
        for rep in range(24):
            n = rng.choice((64, 100, 101, 127, 128))
            s = rng.randrange(0, n - sl + 1)
            ne = rng.randrange(0, k + 3)
            a = rng.randrange(0, ne + 1)
            spec = lambda e: [("sub", e - e // 2), (rng.choice(("del", "ins")), e // 2)]
            add(interior(n), n, s, rep & 1, k, spec(a), spec(ne - a), act=0 if rep % 8 == 7 else 1)
    # the genome's start and the contig ends: windows that end at, one short of, and past the servable range
    for n in (100, 128):
        for loc in (c0, c0 + 1, c0 + 3):
            add(loc, n, 0, 0, KM, ("sub", 1))
        for loc in (0, 1, KM - 1, c0 - 1):          # in the padding before the first contig
            T.append((_rand_bases(rng, n), loc, 0, 0, KM, 1))
        for edge in (end0, c1, n_bases, n_bases + NPAD):
            for off in range(-3, 4):
                loc = edge - (n + MAX_K) + off
                if 0 <= loc and loc + n <= len(bases):
                    add(loc, n, rng.randrange(0, n - sl + 1), off & 1, KM)
    # an N run in the genome under the window
    for off in (-60, -30, -3, 0):
        add(c0 + 5000 + off, 100, 0 if off < -30 else 70, 0, KM)
    rng.shuffle(T)
    # alternate within waves: every fourth task inactive, and a wave's worth of (exact, failing) neighbours
    per = 16 if quad else 32
    for i in range(per):
        n = 101
        loc = interior(n)
        if i % 2:
            T.append((_rand_bases(rng, n), loc, 0, rng.randrange(0, n - sl + 1), KM, 1))
        else:
            add(loc, n, rng.randrange(0, n - sl + 1), i & 2 and 1, rng.randrange(0, KM + 1), act=0 if i % 4 == 0 else 1)
    while len(T) % per:
        n = 100
        add(interior(n), n, 40, 0, KM, ("sub", 2))
    add(interior(100), 100, 33, 1, KM, ("del", 2), ("ins", 1))      # the last wave: a single task
    return T


def expected_filter(task, bases, pieces, n_bases, padding=FILTER_PADDING, seed_len=FILTER_SEED_LEN):
    """-> (encoded word, e1, e2, netIndel of the forward call, of the reverse call)."""
    read, loc, d, s, k, act = task
    n = len(read)
    if not act or not _servable(pieces, n_bases, padding, loc, n + MAX_K):
        return 0, None, None, 0, 0
    rd = revcomp(read) if d else read
    q = b"I" * n
    t = s + seed_len
    e1, n1, _ = oracle_lv_at(1, bases, loc + t, n + MAX_K - t, rd[t:], q[t:], k)
    e2, n2 = -1, 0
    if e1 >= 0:
        e2, n2, _ = oracle_lv_at(-1, bases, loc + s, s + MAX_K, rd[:s][::-1], q[:s], k - e1)
    w = FRES_VALID | (7 if e1 < 0 else e1) << 8 | (7 if e2 < 0 else e2) << 11
    return w, e1, e2, n1, n2
