#!/usr/bin/env python3
"""Regenerate the golden fixtures under tests/golden/ from the REFERENCE itself.

Runs only in the build container (needs /root/reference and oracle/_ref, built by
`make -f oracle/Makefile.ref`).  Inputs are produced by this repo's deterministic
generators; expected outputs come from the reference's own snap-rna indexer and
BaseAligner / LandauVishkin / GenomeIndex::lookupSeed (driven by
oracle/ref_harness.cpp).  Everything written here is data: FASTA/FASTQ inputs and
TSV/JSON expected outputs.

    python3 tests/golden/make_golden.py                  # everything
    python3 tests/golden/make_golden.py --only-multihit  # windowed search / multi-hit runs only
    python3 tests/golden/make_golden.py --only-cigar     # CIGAR calls + SAM records only
    python3 tests/golden/make_golden.py --only-refindex  # reference-built index + seedLen fixtures
    python3 tests/golden/make_golden.py --only-single    # `snap-rna single` end-to-end SAM fixtures
    python3 tests/golden/make_golden.py --only-paired    # Intersecting + Chimeric paired-end aligner runs
    python3 tests/golden/make_golden.py --only-long      # 129..256-base reads + long LV vectors (align_kernel<256>)
    python3 tests/golden/make_golden.py --only-bam       # `snap-rna single ... -o out.bam` records (BAMFormat)
    python3 tests/golden/make_golden.py --only-rna150    # `snap-rna paired` on 2 x 150 pairs (configs[4] length)
    python3 tests/golden/make_golden.py --only-contam    # `snap-rna single|paired ... -ct <contamination index>`
    python3 tests/golden/make_golden.py --only-sorted    # `snap-rna single|paired ... -so` (sorted SAM)
    python3 tests/golden/make_golden.py --only-rna-bench # digest of the reference on bench.py's RNA workload
    python3 tests/golden/make_golden.py --only-single-bench # digest + CPU rate of the reference on bench.py's single-end leg
    python3 tests/golden/make_golden.py --only-rna-bam   # `snap-rna paired ... -o out.bam` records (both RNA sets)
    python3 tests/golden/make_golden.py --only-rna-fs    # `snap-rna paired ... -fs` SAM records (2 x <=101 set)
    python3 tests/golden/make_golden.py --only-paired-edges # paired runs on long / unequal mates, repeats, seeds 16 / 25
    python3 tests/golden/make_golden.py --only-verylong  # single-end reads of 257..500 bases (align_kernel<512>)
"""
import hashlib
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "snap-rnaseq_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import snapgpu  # noqa: E402
from readsets import edge_reads  # noqa: E402
from golden_common import (PARAM_SETS, C1, C2, MULTIHIT_RUNS, PAIRED_RUNS, ref_tsv_to_canonical,  # noqa: E402
                           ref_tsvx_to_canonical, digest)

REF_BIN = os.path.join(ROOT, "oracle", "_ref")
SNAP = os.path.join(REF_BIN, "snap-rna")
HARNESS = os.path.join(REF_BIN, "ref_harness")


def run(cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def ref_index(fasta, outdir):
    shutil.rmtree(outdir, ignore_errors=True)
    run([SNAP, "index", fasta, outdir])


def ref_align(idxdir, fq, params):
    args = [str(params[k]) for k in ("maxHits", "maxK", "numSeeds", "extra")]
    return ref_tsv_to_canonical(run([HARNESS, "align", idxdir, fq] + args))


def write_fastq(path, reads):
    with open(path, "w") as f:
        for i, (b, q) in enumerate(reads):
            f.write(f"@r{i}\n{b}\n+\n{q}\n")


def small_genome_fasta(path):
    """300 kb, 3 contigs, repeat-rich; FASTA with mixed case, N runs and a few
    IUPAC bytes (FASTA.cpp:104-116 keeps those upper-cased)."""
    g = snapgpu.Genome.synthetic(300_000, seed=7, n_contigs=3, n_repeat_families=40, n_run_fraction=0.003)
    tmp = path + ".tmp"
    g.write_fasta(tmp)
    rng = random.Random(5)
    out = []
    for line in open(tmp):
        if not line.startswith(">"):
            s = list(line.rstrip("\n"))
            if rng.random() < 0.02:
                s[rng.randrange(len(s))] = rng.choice("RYKM")
            s = "".join(s)
            if rng.random() < 0.05:
                s = s.lower()
            line = s + "\n"
        out.append(line)
    os.remove(tmp)
    with open(path, "w") as f:
        f.writelines(out)


def search_windows(n, default_tsv, n_bases, seed=23):
    """Per-read (radius, location, direction) for the windowed AlignRead: unconstrained,
    windows around the reference's own unconstrained answer (same and opposite
    direction), random windows, and saturating ones (BaseAligner.cpp:596-602)."""
    rng = random.Random(seed)
    best = []
    for line in open(default_tsv):
        x = line.split("\t")
        best.append((int(x[2]), int(x[3])))
    rows = []
    for i in range(n):
        loc, d = best[i]
        kind = rng.randrange(6)
        if kind == 0 or (kind in (1, 2) and loc == 0xFFFFFFFF):
            rows.append((0, 0, 0))
        elif kind in (1, 2):
            rad = rng.choice([1, 30, 200, 5000])
            c = max(0, loc + rng.randint(-rad, rad))
            rows.append((rad, c, d if kind == 1 else 1 - d))
        elif kind == 3:
            rows.append((rng.choice([1000, 50000]), rng.randrange(n_bases), rng.randrange(2)))
        elif kind == 4:
            rows.append((rng.choice([0xFFFFFFF0, 4000000000]), rng.randrange(n_bases), rng.randrange(2)))
        else:
            rows.append((rng.choice([100, 3000]), rng.randrange(200), rng.randrange(2)))
    return rows


def multihit_fixtures(work):
    """Windowed search + multi-hit export (BaseAligner.h:73-86) on the small genome."""
    fa = os.path.join(HERE, "small.fa")
    idxdir = os.path.join(work, "small_idx_mh")
    ref_index(fa, idxdir)
    g = snapgpu.Genome.from_fasta(fa, 500)
    fq = os.path.join(HERE, "small_reads.fq")
    n = sum(1 for _ in open(fq)) // 4
    rows = search_windows(n, os.path.join(HERE, "expected_small_default.tsv"), g.n_bases)
    sp = os.path.join(HERE, "small_search.tsv")
    with open(sp, "w") as f:
        f.writelines(f"{a}\t{b}\t{c}\n" for a, b, c in rows)
    for name, (maxget, pset) in MULTIHIT_RUNS.items():
        params = PARAM_SETS[pset]
        args = [str(params[k]) for k in ("maxHits", "maxK", "numSeeds", "extra")]
        out = run([HARNESS, "alignx", idxdir, fq, sp, str(maxget)] + args)
        with open(os.path.join(HERE, f"expected_small_{name}.tsv"), "w") as f:
            f.write(ref_tsvx_to_canonical(out))


def read_fastq(path):
    lines = open(path).read().split("\n")
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def cigar_fixtures(work):
    """CIGAR / SAM record: the reference's own SAM writer
    (FileFormat::SAM[useM]->writeRead, SAM.cpp:1007-1155) over BaseAligner's results on
    the small genome, and LandauVishkinWithCigar as computeCigarString calls it
    (SAM.cpp:1162-1230) at the aligned location and at perturbed / random locations
    (large edit distances, indel-heavy backtraces, '*' results, genome ends)."""
    import gzip
    fa = os.path.join(HERE, "small.fa")
    idxdir = os.path.join(work, "small_idx_cig")
    ref_index(fa, idxdir)
    g = snapgpu.Genome.from_fasta(fa, 500)
    fq = os.path.join(HERE, "small_reads.fq")
    sam = run([HARNESS, "sam", idxdir, fq])
    with open(os.path.join(HERE, "expected_small.sam.gz"), "wb") as f:   # mtime 0: reproducible bytes
        f.write(gzip.compress(sam.encode(), compresslevel=9, mtime=0))
    # the reference FASTQ reader's default clipping (ClipFrontAndBack, AlignerOptions.cpp:48,
    # FASTQ.cpp:250): the clipped reads are aligned, the SAM line carries S ops + unclipped SEQ
    sam3 = run([HARNESS, "sam", idxdir, fq, "300", "14", "25", "2", "3"])
    with open(os.path.join(HERE, "expected_small_clipped.sam.gz"), "wb") as f:
        f.write(gzip.compress(sam3.encode(), compresslevel=9, mtime=0))
    reads = read_fastq(fq)
    res = [l.split("\t") for l in open(os.path.join(HERE, "expected_small_default.tsv")).read().splitlines()]
    rng = random.Random(31)
    nb = g.n_bases
    rows = []
    for (rid, b, q), r in zip(reads, res):
        result, loc, d = int(r[1]), int(r[2]), int(r[3])
        if loc != 0xFFFFFFFF:
            rows.append((loc, 0 if result == 0 else d, rng.randrange(2), b))
            for _ in range(2):
                dl = rng.choice([rng.randrange(-4, 5), rng.randrange(-35, 36)])
                pl = max(0, loc + dl)
                rows.append((pl, d if rng.random() < 0.8 else 1 - d, rng.randrange(2), b))
        if rng.random() < 0.15:
            rows.append((rng.choice([0, 1, nb - len(b), nb - len(b) + 1, nb - 50, nb + 99, rng.randrange(nb)]),
                         rng.randrange(2), rng.randrange(2), b))
    inp = os.path.join(HERE, "cigar_calls.tsv")
    with open(inp, "w") as f:
        f.writelines(f"{a}\t{b}\t{c}\t{d}\n" for a, b, c, d in rows)
    with open(os.path.join(HERE, "expected_cigar.tsv"), "w") as f:
        f.write(run([HARNESS, "cigar", idxdir, inp]))
    # SAMFormat::writeHeader (SAM.cpp:700-800), unsorted and sorted
    for srt in (0, 1):
        with open(os.path.join(HERE, f"expected_small_header{srt}.sam"), "w") as f:
            f.write(run([HARNESS, "samheader", idxdir, str(srt), "1.0dev.66", "snap-rna", "single", "idx",
                         "reads.fq", "-o", "out.sam"]))


SEED_LENS = (16, 22, 25)


def refindex_fixtures(work):
    """(1) The reference's own on-disk index of small.fa (`snap-rna index`, seed 20, slack 0.3),
    committed as a gzipped tar: the exact input GenomeIndex::loadFromDirectory
    (GenomeIndex.cpp:845-963) and our snapgpu_index_load read.  (2) The reference's AlignRead
    outputs at seed lengths 16, 22 and 25 (`snap-rna index -s N`): these pin the
    GetWrappedNextSeedToTest tables of SeedSequencer.h:28-287 and the 1 / 4096 / 262144-table
    layouts."""
    import tarfile
    import io
    import gzip
    fa = os.path.join(HERE, "small.fa")
    fq = os.path.join(HERE, "small_reads.fq")
    idxdir = os.path.join(work, "small_ref_idx")
    ref_index(fa, idxdir)
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w") as t:
        for fn in sorted(os.listdir(idxdir)):
            info = t.gettarinfo(os.path.join(idxdir, fn), arcname=fn)
            info.mtime = 0
            info.uid = info.gid = 0
            info.uname = info.gname = ""
            with open(os.path.join(idxdir, fn), "rb") as f:
                t.addfile(info, f)
    with open(os.path.join(HERE, "small_ref_index.tar.gz"), "wb") as f:
        f.write(gzip.compress(buf.getvalue(), compresslevel=9, mtime=0))
    for L in SEED_LENS:
        d = os.path.join(work, f"small_idx_s{L}")
        shutil.rmtree(d, ignore_errors=True)
        run([SNAP, "index", fa, d, "-s", str(L)])
        with open(os.path.join(HERE, f"expected_small_seed{L}.tsv"), "w") as f:
            f.write(ref_align(d, fq, PARAM_SETS["default"]))


def small_gtf(path, seqs, rng):
    """Genes on small.fa: 2-5 exons, alternative transcripts that skip exons (shared exons and
    introns), an exon abutting the next (zero-length intron), a transcript on a chromosome the
    genome lacks (skipped by BuildTranscriptome), and non-exon lines (ignored by Parse)."""
    lines = ["#!genome-build synthetic", "#!annotation for tests/golden/small.fa"]
    chrs = list(seqs)
    for g in range(12):
        c = chrs[g % len(chrs)]
        L = len(seqs[c])
        p = rng.randrange(2000, L - 30000)
        exons = []
        for e in range(rng.randrange(2, 6)):
            ln = rng.randrange(60, 400)
            exons.append((p, p + ln - 1))
            p += ln + (0 if (g == 3 and e == 0) else rng.randrange(150, 2500))
        lines.append(f'{c}\tsrc\tgene\t{exons[0][0]}\t{exons[-1][1]}\t.\t+\t.\tgene_id "G{g}"; gene_name "GENE{g}";')
        for t in range(rng.randrange(1, 4)):
            use = exons if t == 0 else [x for k, x in enumerate(exons) if k == 0 or k == len(exons) - 1 or rng.random() < 0.5]
            for a, b in use:
                lines.append(f'{c}\tsrc\texon\t{a}\t{b}\t.\t{"+-"[g % 2]}\t.\tgene_id "G{g}"; transcript_id "T{g}.{t}"; '
                             f'gene_name "GENE{g}"; transcript_name "GENE{g}-{t}";')
    lines.append('chrUn\tsrc\texon\t100\t400\t.\t+\t.\tgene_id "GX"; transcript_id "TX.0";')
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines


def single_reads(path, seqs, gtf_lines, rng):
    """Reads for the end-to-end run: from transcript pre-mRNA spans (the transcriptome the
    reference builds) around exon/intron boundaries, from anywhere in the genome, both strands;
    '#' runs at the ends (clipping), low-quality reads, N-rich reads, short reads, random reads."""
    comp = str.maketrans("ACGTN", "TGCAN")
    ex = [l.split("\t") for l in gtf_lines if "\texon\t" in l and not l.startswith("chrUn")]
    reads = []
    for i in range(1200):
        u = rng.random()
        if u < 0.55:
            f = rng.choice(ex)
            c, a, b = f[0], int(f[3]), int(f[4])
            pos = rng.randrange(max(0, a - 160), b + 60) - 1
        elif u < 0.95:
            c = rng.choice(list(seqs))
            pos = rng.randrange(0, len(seqs[c]) - 200)
        else:
            c, pos = None, 0
        L = rng.choice([100, 100, 100, 101, 120, 75, 60, 45])
        s = "".join(rng.choice("ACGT") for _ in range(L)) if c is None else seqs[c][pos:pos + L]
        s = list(s)
        for _ in range(rng.choice([0, 0, 1, 2, 3, 6])):
            s[rng.randrange(len(s))] = rng.choice("ACGT")
        if rng.random() < 0.05:
            j = rng.randrange(5, len(s) - 5)
            s = s[:j] + s[j + rng.randrange(1, 4):] if rng.random() < 0.5 else s[:j] + list("ACG"[:rng.randrange(1, 4)]) + s[j:]
        s = "".join(s)
        if rng.random() < 0.5:
            s = s.translate(comp)[::-1]
        q = ["I"] * len(s)
        r = rng.random()
        if r < 0.08:
            q = [rng.choice("#%+5") for _ in s]
        elif r < 0.25:
            for j in range(rng.randrange(1, 12)):
                q[-1 - j] = "#"
            for j in range(rng.randrange(0, 5)):
                q[j] = "#"
        elif r < 0.3:
            q = [rng.choice("I?5") for _ in s]
        if rng.random() < 0.03:
            s = "".join("N" if rng.random() < 0.25 else ch for ch in s)
        reads.append((f"sr{i} len={len(s)}", s, "".join(q)))
    with open(path, "w") as f:
        for n, s, q in reads:
            f.write(f"@{n}\n{s}\n+\n{q}\n")


def single_fixtures(work):
    """`snap-rna single <genome> <transcriptome> <gtf> <reads> -t 1 -o out.sam` (the product
    path, SingleAligner.cpp:141-320), default options and -M; plus the reference's
    transcriptome FASTA (GTFReader::BuildTranscriptome) for the same GTF."""
    import gzip
    rng = random.Random(41)
    fa = os.path.join(HERE, "small.fa")
    seqs, name = {}, None
    for line in open(fa):
        line = line.strip()
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(line.upper())
    seqs = {k: "".join(v) for k, v in seqs.items()}
    gtf = os.path.join(HERE, "small.gtf")
    lines = small_gtf(gtf, seqs, rng)
    fq = os.path.join(HERE, "single_reads.fq")
    single_reads(fq, seqs, lines, rng)
    gidx = os.path.join(work, "gidx")
    ref_index(fa, gidx)
    twd = os.path.join(work, "tx")
    os.makedirs(twd, exist_ok=True)
    run([SNAP, "transcriptome", gtf, fa, "tidx", "-O1000"], cwd=twd)
    with open(os.path.join(twd, "transcriptome.fa"), "rb") as src, \
            open(os.path.join(HERE, "expected_transcriptome.fa.gz"), "wb") as dst:
        dst.write(gzip.compress(src.read(), compresslevel=9, mtime=0))
    for tag, extra in (("", []), ("_M", ["-M"])):
        out = os.path.join(work, f"out{tag}.sam")
        run([SNAP, "single", gidx, os.path.join(twd, "tidx"), gtf, fq, "-t", "1", "-o", out] + extra, cwd=work)
        with open(out, "rb") as src, open(os.path.join(HERE, f"expected_single{tag}.sam.gz"), "wb") as dst:
            dst.write(gzip.compress(src.read(), compresslevel=9, mtime=0))
        if not tag:   # GTFReader::WriteReadCounts after the run (gene counts from FilterSingle)
            with open(os.path.join(HERE, "expected_single.counts.txt"), "w") as dst:
                for c in ("transcript_id", "transcript_name", "gene_id", "gene_name", "junction_id", "junction_name"):
                    dst.write(f"## {c}\n")
                    dst.write(open(os.path.join(work, f"out.{c}.counts.txt")).read())


def paired_reads(path0, path1, seqs, rng):
    """Read pairs over small.fa: proper pairs (either mate first, either strand, inserts
    150-700), with substitutions/indels; overlapping mates (insert < minSpacing); inserts past
    maxSpacing; chimeric pairs (mates from unrelated places); one or both mates random; short
    mates (< 50, IntersectingPairedEndAligner.cpp:186 / ChimericPairedEndAligner.cpp:61);
    N-rich mates (> maxK Ns over the pair, :226); same-orientation mates; 150-base mates."""
    comp = str.maketrans("ACGTN", "TGCAN")
    rc = lambda x: x.translate(comp)[::-1]
    names = list(seqs)

    def mutate(s):
        s = list(s)
        for _ in range(rng.choice([0, 0, 0, 1, 2, 3, 5, 8])):
            s[rng.randrange(len(s))] = rng.choice("ACGT")
        if rng.random() < 0.08:
            j = rng.randrange(5, len(s) - 5)
            s = s[:j] + s[j + rng.randrange(1, 4):] if rng.random() < 0.5 else s[:j] + list("TGA"[:rng.randrange(1, 4)]) + s[j:]
        return "".join(s)

    def rand_seq(L):
        return "".join(rng.choice("ACGT") for _ in range(L))

    def frag_pair(L0, L1, ins):
        c = rng.choice(names)
        g = seqs[c]
        pos = rng.randrange(0, max(1, len(g) - ins - 1))
        f = g[pos:pos + ins]
        if rng.random() < 0.5:
            f = rc(f)
        return f[:L0], rc(f[len(f) - L1:])

    pairs = []
    for i in range(2400):
        u = rng.random()
        L0 = L1 = rng.choice([101, 101, 101, 100, 90, 150, 75, 60])
        if u < 0.62:
            a, b = frag_pair(L0, L1, rng.randrange(max(L0, 150), 700))
        elif u < 0.67:
            a, b = frag_pair(L0, L1, rng.randrange(L0, L0 + 40))          # mates overlap: within minSpacing
        elif u < 0.71:
            a, b = frag_pair(L0, L1, rng.randrange(1050, 4000))           # beyond maxSpacing
        elif u < 0.79:
            a, _ = frag_pair(L0, L1, 400)                                  # chimeric
            _, b = frag_pair(L0, L1, 400)
        elif u < 0.84:
            a, b = frag_pair(L0, L1, 400)
            if rng.random() < 0.5:
                a = rand_seq(L0)
            else:
                b = rand_seq(L1)
        elif u < 0.86:
            a, b = rand_seq(L0), rand_seq(L1)
        elif u < 0.90:
            a, b = frag_pair(L0, L1, 400)
            if rng.random() < 0.5:
                a = a[:rng.randrange(20, 50)]
            else:
                b = b[:rng.randrange(20, 50)]
            if rng.random() < 0.2:
                a, b = a[:40], b[:45]
        elif u < 0.93:
            a, b = frag_pair(L0, L1, 400)
            a = "".join("N" if rng.random() < 0.12 else ch for ch in a)
        elif u < 0.96:
            a, b = frag_pair(L0, L1, 400)
            b = rc(b)                                                      # same orientation
        else:
            a, b = frag_pair(L0, L1, rng.randrange(200, 500))
            a, b = b, a
        if rng.random() < 0.5:
            a, b = b, a
        a, b = mutate(a) if len(a) > 12 else a, mutate(b) if len(b) > 12 else b
        qa, qb = ["I"] * len(a), ["I"] * len(b)
        if rng.random() < 0.1:
            qa = [rng.choice("#+5?I") for _ in a]
        pairs.append((a, "".join(qa), b, "".join(qb)))
    with open(path0, "w") as f0, open(path1, "w") as f1:
        for i, (a, qa, b, qb) in enumerate(pairs):
            f0.write(f"@p{i}/1\n{a}\n+\n{qa}\n")
            f1.write(f"@p{i}/2\n{b}\n+\n{qb}\n")


def paired_fixtures(work):
    """`ref_harness paired`: IntersectingPairedEndAligner::align and ChimericPairedEndAligner::align
    (constructed as PairedAligner.cpp:462-482) for every pair, under PAIRED_RUNS."""
    rng = random.Random(61)
    fa = os.path.join(HERE, "small.fa")
    seqs, name = {}, None
    for line in open(fa):
        line = line.strip()
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(line.upper())
    seqs = {k: "".join(v) for k, v in seqs.items()}
    fq0, fq1 = os.path.join(HERE, "paired_1.fq"), os.path.join(HERE, "paired_2.fq")
    paired_reads(fq0, fq1, seqs, rng)
    idx = os.path.join(work, "pidx")
    ref_index(fa, idx)
    for name, p in PAIRED_RUNS.items():
        args = [str(p[k]) for k in ("maxHits", "maxK", "numSeeds", "extra", "minSpacing", "maxSpacing", "maxBigHits")]
        with open(os.path.join(HERE, f"expected_paired_{name}.tsv"), "w") as f:
            f.write(run([HARNESS, "paired", idx, fq0, fq1] + args))


HARNESS_RNA = os.path.join(REF_BIN, "ref_harness_rna")


def multihit_alias_fixtures(work):
    """maxHitsToGet 1000 (the RNA paired path's transcriptome call, PairedAligner.cpp:584) on a
    genome holding one 150-base element 700 times exactly, 700 times with one substitution and
    400 times with two: more than 512 hits at one distance, so the reference's per-distance rows
    (hitLocations[MAX_K][512], BaseAligner.h:148-151) overflow into each other.  Paired CLI
    aligner parameters (maxHits 16000, maxK 15, 8 seeds, extra 2), no search window."""
    rng = random.Random(77)
    elem = "".join(rng.choice("ACGT") for _ in range(150))
    sub = lambda s, i: s[:i] + {"A": "C", "C": "G", "G": "T", "T": "A"}[s[i]] + s[i + 1:]
    copies = [elem] * 700 + [sub(elem, 75)] * 700 + [sub(sub(elem, 40), 110)] * 400
    rng.shuffle(copies)
    seqs = []
    for c in range(3):
        parts = ["".join(rng.choice("ACGT") for _ in range(5000))]
        for k in copies[c * 600:(c + 1) * 600]:
            parts.append(k if rng.random() < 0.5 else k[::-1].translate(str.maketrans("ACGT", "TGCA")))
            parts.append("".join(rng.choice("ACGT") for _ in range(rng.randrange(20, 60))))
        seqs.append("".join(parts))
    fa = os.path.join(HERE, "repeat.fa")
    with open(fa, "w") as f:
        for c, sq in enumerate(seqs):
            f.write(f">rep{c}\n")
            f.writelines(sq[i:i + 70] + "\n" for i in range(0, len(sq), 70))
    rc = lambda x: x[::-1].translate(str.maketrans("ACGT", "TGCA"))
    reads = []
    for i in range(24):
        a = rng.randrange(0, 50)
        r = elem[a:a + 100]
        if i % 3 == 1:
            r = sub(r, 60)
        if i % 2:
            r = rc(r)
        reads.append((r, "I" * len(r)))
    for i in range(8):   # anchored outside the element as well
        c = rng.randrange(3)
        p0 = rng.randrange(0, 4800)
        r = seqs[c][p0:p0 + 100]
        reads.append((r, "I" * len(r)))
    fq = os.path.join(HERE, "repeat_reads.fq")
    write_fastq(fq, reads)
    sp = os.path.join(work, "nosearch.tsv")
    with open(sp, "w") as f:
        f.writelines("0\t0\t0\n" for _ in reads)
    idxdir = os.path.join(work, "repeat_idx")
    run([SNAP, "index", fa, idxdir, "-O1000"])   # a repeat this dense needs the larger overflow space
    out = run([HARNESS, "alignx", idxdir, fq, sp, "1000", "16000", "15", "8", "2"])
    with open(os.path.join(HERE, "expected_repeat_mh1000.tsv"), "w") as f:
        f.write(ref_tsvx_to_canonical(out))


def charseeds_fixtures(work):
    """`ref_harness_rna charseeds`: BaseAligner::CharacterizeSeeds (BaseAligner.cpp:206-508) of
    the partial aligner (PairedAligner.cpp:518-527: maxHits 300, maxK 15, 12 seeds) over every
    read of paired_1.fq / paired_2.fq and single_reads.fq, on the reference's index of small.fa,
    plus a tight variant (maxHits 20, 4 seeds) that makes popular seeds common."""
    import gzip
    fa = os.path.join(HERE, "small.fa")
    idx = os.path.join(work, "csidx")
    ref_index(fa, idx)
    for tag, args in (("", []), ("_tight", ["20", "15", "4", "2"])):
        out = []
        for fq in ("paired_1.fq", "paired_2.fq", "single_reads.fq"):
            out.append(run([HARNESS_RNA, "charseeds", idx, os.path.join(HERE, fq)] + args))
        with open(os.path.join(HERE, f"expected_charseeds{tag}.tsv.gz"), "wb") as f:
            f.write(gzip.compress("".join(out).encode(), compresslevel=9, mtime=0))


RNA_BLOCK = 200
COUNT_FILES = ("transcript_id", "transcript_name", "gene_id", "gene_name", "junction_id", "junction_name")


def rna_paired_reads(path0, path1, seqs, gtf_path, rng, n_pairs=3000, lengths=(101, 101, 100, 100, 90, 75)):
    """Read pairs for `snap-rna paired` (PairedAligner.cpp:405-668): mates from spliced mRNAs
    (crossing exon junctions) and from pre-mRNA spans (the transcriptome the reference indexes),
    intergenic pairs, chimeras between genes on one chromosome and on two, same-orientation
    mates, one or both mates random, short / N-rich / low-quality mates, mutated mates."""
    comp = str.maketrans("ACGTN", "TGCAN")
    rc = lambda x: x.translate(comp)[::-1]
    tx = {}
    for line in open(gtf_path):
        f = line.rstrip("\n").split("\t")
        if len(f) < 9 or f[2] != "exon" or f[0] not in seqs:
            continue
        tid = f[8].split('transcript_id "')[1].split('"')[0]
        tx.setdefault(tid, []).append((f[0], int(f[3]), int(f[4])))
    spliced, premrna = [], []
    for t, ex in sorted(tx.items()):
        ex.sort(key=lambda e: e[1])
        c = ex[0][0]
        spliced.append((c, "".join(seqs[c][a - 1:b] for _, a, b in ex)))
        premrna.append((c, seqs[c][ex[0][1] - 1:ex[-1][2]]))
    names = list(seqs)

    def mutate(s):
        s = list(s)
        for _ in range(rng.choice([0, 0, 0, 1, 2, 4])):
            s[rng.randrange(len(s))] = rng.choice("ACGT")
        return "".join(s)

    def rand_seq(L):
        return "".join(rng.choice("ACGT") for _ in range(L))

    def frag(src, L0, L1, ins):
        ins = max(ins, L0, L1)
        if len(src) <= ins:
            ins = len(src)
        p = rng.randrange(0, len(src) - ins + 1)
        f = src[p:p + ins]
        if rng.random() < 0.5:
            f = rc(f)
        return f[:L0], rc(f[len(f) - L1:])

    def genomic(L0, L1, ins):
        c = rng.choice(names)
        return frag(seqs[c], L0, L1, ins)

    def gene_mate(L, pool=None):
        c, sq = rng.choice(pool or spliced)
        a, _ = frag(sq, L, L, L)
        return c, a

    pairs = []
    for i in range(n_pairs):
        u = rng.random()
        L0 = L1 = rng.choice(list(lengths))
        if u < 0.30:
            a, b = frag(rng.choice(spliced)[1], L0, L1, rng.randrange(150, 450))
        elif u < 0.45:
            a, b = frag(rng.choice(premrna)[1], L0, L1, rng.randrange(150, 600))
        elif u < 0.55:
            a, b = genomic(L0, L1, rng.randrange(150, 700))
        elif u < 0.65:   # chimera within one chromosome (two genes)
            c0, a = gene_mate(L0)
            same = [x for x in spliced if x[0] == c0]
            _, b = gene_mate(L1, same)
        elif u < 0.73:   # chimera across chromosomes
            c0, a = gene_mate(L0)
            other = [x for x in spliced if x[0] != c0] or spliced
            _, b = gene_mate(L1, other)
        elif u < 0.78:   # same orientation
            a, b = frag(rng.choice(spliced + premrna)[1], L0, L1, rng.randrange(150, 400))
            b = rc(b)
        elif u < 0.86:   # one mate random
            a, b = frag(rng.choice(spliced)[1], L0, L1, 300)
            if rng.random() < 0.5:
                a = rand_seq(L0)
            else:
                b = rand_seq(L1)
        elif u < 0.89:
            a, b = rand_seq(L0), rand_seq(L1)
        elif u < 0.92:   # genomic pair far apart on one chromosome (past maxSpacing)
            a, b = genomic(L0, L1, rng.randrange(1500, 20000))
        elif u < 0.95:
            a, b = frag(rng.choice(spliced)[1], L0, L1, 300)
            if rng.random() < 0.5:
                a = a[:rng.randrange(30, 60)]
            else:
                a = "".join("N" if rng.random() < 0.2 else ch for ch in a)
        else:
            a, b = frag(rng.choice(premrna)[1], L0, L1, rng.randrange(150, 400))
        if rng.random() < 0.5:
            a, b = b, a
        a, b = mutate(a), mutate(b)
        # small.fa's IUPAC codes: the FASTQ reader takes a record starting with one for garbage
        # (FASTQ.cpp:241), so mates carry ACGTN only
        a, b = ("".join(ch if ch in "ACGTN" else "A" for ch in x) for x in (a, b))
        qa, qb = ["I"] * len(a), ["I"] * len(b)
        r = rng.random()
        if r < 0.05:
            qa = [rng.choice("#+5?I") for _ in a]
        elif r < 0.15:
            for j in range(rng.randrange(1, 10)):
                qb[-1 - j] = "#"
        pairs.append((a, "".join(qa), b, "".join(qb)))
    with open(path0, "w") as f0, open(path1, "w") as f1:
        for i, (a, qa, b, qb) in enumerate(pairs):
            f0.write(f"@rp{i}/1\n{a}\n+\n{qa}\n")
            f1.write(f"@rp{i}/2\n{b}\n+\n{qb}\n")


RNA_SETS = {
    # name: (rng seed, pairs, mate lengths, file stem)
    "": (83, 3000, (101, 101, 100, 100, 90, 75), "rna"),
    # BASELINE configs[4] read length: 2 x 150 (align_kernel<256>, paired_kernel<256>, 150-b CIGARs)
    "150": (151, 2000, (150, 150, 150, 150, 149, 140, 120), "rna150"),
}


def rna_paired_fixtures(work, variant=""):
    """`snap-rna paired <genome> <transcriptome> <gtf> r1.fq r2.fq -t 1 -o out.sam` (the RNA
    paired product path, PairedAligner.cpp:405-689; BaseAligner.cpp at -O0, see
    oracle/Makefile.ref): the SAM file and the six read-count files GTFReader::WriteReadCounts
    writes (GTFReader.cpp:1710-1772).  variant "150": 2 x 150 pairs (configs[4]'s read length)."""
    import gzip
    seed, n_pairs, lengths, stem = RNA_SETS[variant]
    rng = random.Random(seed)
    fa = os.path.join(HERE, "small.fa")
    seqs, name = {}, None
    for line in open(fa):
        line = line.strip()
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(line.upper())
    seqs = {k: "".join(v) for k, v in seqs.items()}
    gtf = os.path.join(HERE, "small.gtf")
    fq0, fq1 = os.path.join(HERE, f"{stem}_1.fq"), os.path.join(HERE, f"{stem}_2.fq")
    rna_paired_reads(fq0, fq1, seqs, gtf, rng, n_pairs, lengths)
    gidx = os.path.join(work, "gidx")
    ref_index(fa, gidx)
    twd = os.path.join(work, "tx")
    os.makedirs(twd, exist_ok=True)
    run([SNAP, "transcriptome", gtf, fa, "tidx", "-O1000"], cwd=twd)
    # The reference segfaults at the end of a run in GTFReader::AnalyzeReadIntervals (the
    # interval-clustering report, GTFReader.cpp:1774-1838 -- not restated here) once enough
    # overlapping read-pair intervals accumulate.  So the pairs are aligned in blocks of
    # RNA_BLOCK (each block is its own `snap-rna paired` run, SAM bodies concatenated, count
    # files kept per block), and a pair whose block still crashes on its own is left out.
    recs = [open(x).read().splitlines() for x in (fq0, fq1)]
    n = len(recs[0]) // 4

    def attempt(idx, d, extra=(), out="try"):
        for k in range(2):
            with open(os.path.join(d, f"{out}_{k}.fq"), "w") as f:
                f.write("".join("\n".join(recs[k][4 * i:4 * i + 4]) + "\n" for i in idx))
        r = subprocess.run([SNAP, "paired", gidx, os.path.join(twd, "tidx"), gtf, os.path.join(d, f"{out}_0.fq"),
                            os.path.join(d, f"{out}_1.fq"), "-t", "1", "-o", os.path.join(d, f"{out}.sam")] + list(extra),
                           capture_output=True, cwd=d)
        return r.returncode == 0

    if variant:
        return _rna_blocks_bisect(recs, n, attempt, work, fq0, fq1, stem)
    drop = []
    for c in range(0, n, RNA_BLOCK):
        block = list(range(c, min(n, c + RNA_BLOCK)))
        if not attempt(block, work):
            drop += [i for i in block if not attempt([i], work)]
    keep = [i for i in range(n) if i not in set(drop)]
    for k, x in enumerate((fq0, fq1)):
        with open(x, "w") as f:
            f.write("".join("\n".join(recs[k][4 * i:4 * i + 4]) + "\n" for i in keep))
    recs = [open(x).read().splitlines() for x in (fq0, fq1)]
    n = len(recs[0]) // 4
    if drop:
        print("pairs left out (the reference crashes in AnalyzeReadIntervals):", drop)
    for tag, extra in (("", []), ("_M", ["-M"])):
        body, counts = [], []
        for bi, c in enumerate(range(0, n, RNA_BLOCK)):
            assert attempt(range(c, min(n, c + RNA_BLOCK)), work, extra, out=f"blk{tag}")
            lines = open(os.path.join(work, f"blk{tag}.sam")).read().splitlines(keepends=True)
            if bi == 0:
                body += [l for l in lines if l.startswith("@")]
            body += [l for l in lines if not l.startswith("@")]
            for cf in COUNT_FILES:
                counts.append(f"## block {bi} {cf}\n")
                counts.append(open(os.path.join(work, f"blk{tag}.{cf}.counts.txt")).read())
        with open(os.path.join(HERE, f"expected_{stem}_paired{tag}.sam.gz"), "wb") as dst:
            dst.write(gzip.compress("".join(body).encode(), compresslevel=9, mtime=0))
        if not tag:
            with open(os.path.join(HERE, f"expected_{stem}_paired.counts.txt"), "w") as dst:
                dst.write("".join(counts))


def contamination_fixtures(work):
    """`snap-rna single|paired ... -ct <contamination index>` (SingleAligner.cpp:205-293,
    PairedAligner.cpp:487-645, ContaminationFilter.cpp): reads left NotFound by the filter are
    aligned to the contamination index and every aligned contaminant counted by contig;
    ContaminationFilter::Write leaves `<output prefix>.contaminants.txt` (contig, count; by count,
    descending).  contam.fa: five random contigs (the counts tie on purpose); the read sets mix
    reads of the existing single / 2 x 150 RNA fixtures with reads and pairs from the contigs
    (mutated, either strand).  The SAM output must not change with -ct (checked here)."""
    import gzip
    rng = random.Random(1907)
    comp = str.maketrans("ACGT", "TGCA")
    rc = lambda x: x.translate(comp)[::-1]
    contigs = {f"cont{i}": "".join(rng.choice("ACGT") for _ in range(ln))
               for i, ln in enumerate((6000, 9000, 4000, 7000, 5000), 1)}
    cfa = os.path.join(HERE, "contam.fa")
    with open(cfa, "w") as f:
        for name, seq in contigs.items():
            f.write(f">{name}\n")
            f.write("".join(seq[i:i + 60] + "\n" for i in range(0, len(seq), 60)))
    cidx = os.path.join(work, "cidx")
    ref_index(cfa, cidx)

    def mutate(x):
        x = list(x)
        for _ in range(rng.choice([0, 0, 1, 2, 3])):
            x[rng.randrange(len(x))] = rng.choice("ACGT")
        return "".join(x)

    # per contig how many reads / pairs: equal counts for some contigs (the sort's ties)
    plan = {"cont1": 20, "cont2": 35, "cont3": 20, "cont4": 8, "cont5": 20}
    fa = os.path.join(HERE, "small.fa")
    gidx = os.path.join(work, "gidx")
    ref_index(fa, gidx)
    gtf = os.path.join(HERE, "small.gtf")
    twd = os.path.join(work, "tx")
    os.makedirs(twd, exist_ok=True)
    run([SNAP, "transcriptome", gtf, fa, "tidx", "-O1000"], cwd=twd)
    # single: 300 reads of single_reads.fq + contaminant reads, shuffled in
    recs = open(os.path.join(HERE, "single_reads.fq")).read().splitlines()
    base = [recs[4 * i:4 * i + 4] for i in range(300)]
    extra = []
    for name, k in plan.items():
        for j in range(k):
            p = rng.randrange(0, len(contigs[name]) - 100)
            x = mutate(contigs[name][p:p + 100])
            extra.append([f"@c_{name}_{j}", x if rng.random() < 0.5 else rc(x), "+", "I" * 100])
    allr = base + extra
    rng.shuffle(allr)
    sfq = os.path.join(HERE, "contam_single.fq")
    with open(sfq, "w") as f:
        f.write("".join("\n".join(r) + "\n" for r in allr))
    outs = {}
    for tag, extra_args in (("plain", []), ("x", ["-ct", cidx])):
        out = os.path.join(work, f"cs_{tag}.sam")
        run([SNAP, "single", gidx, os.path.join(twd, "tidx"), gtf, sfq, "-t", "1", "-o", out] + extra_args, cwd=work)
        outs[tag] = [l for l in open(out).read().splitlines() if not l.startswith("@PG")]
    assert outs["plain"] == outs["x"], "the SAM output changed with -ct"
    with open(os.path.join(HERE, "expected_contam_single.sam.gz"), "wb") as dst:
        dst.write(gzip.compress(open(os.path.join(work, "cs_x.sam"), "rb").read(), compresslevel=9, mtime=0))
    shutil.copy(os.path.join(work, "cs_x.contaminants.txt"), os.path.join(HERE, "expected_contam_single.contaminants.txt"))
    # paired: 150 pairs of the 2 x 150 RNA set + contaminant pairs (insert 250-450, FR)
    r0 = open(os.path.join(HERE, "rna150_1.fq")).read().splitlines()
    r1 = open(os.path.join(HERE, "rna150_2.fq")).read().splitlines()
    pairs = [(r0[4 * i:4 * i + 4], r1[4 * i:4 * i + 4]) for i in range(150)]
    for name, k in plan.items():
        for j in range(k):
            ins = rng.randrange(250, 450)
            p = rng.randrange(0, len(contigs[name]) - ins)
            frag = contigs[name][p:p + ins]
            a, b = mutate(frag[:150]), mutate(rc(frag)[:150])
            if rng.random() < 0.5:
                a, b = b, a
            nm = f"@cp_{name}_{j}"
            pairs.append(([nm + "/1", a, "+", "I" * 150], [nm + "/2", b, "+", "I" * 150]))
    rng.shuffle(pairs)
    pfq = [os.path.join(HERE, f"contam_paired_{k}.fq") for k in (1, 2)]
    for k in range(2):
        with open(pfq[k], "w") as f:
            f.write("".join("\n".join(pr[k]) + "\n" for pr in pairs))
    outs = {}
    for tag, extra_args in (("plain", []), ("x", ["-ct", cidx])):
        out = os.path.join(work, f"cp_{tag}.sam")
        run([SNAP, "paired", gidx, os.path.join(twd, "tidx"), gtf, pfq[0], pfq[1], "-t", "1", "-o", out] + extra_args,
            cwd=work)
        outs[tag] = [l for l in open(out).read().splitlines() if not l.startswith("@PG")]
    assert outs["plain"] == outs["x"], "the SAM output changed with -ct"
    with open(os.path.join(HERE, "expected_contam_paired.sam.gz"), "wb") as dst:
        dst.write(gzip.compress(open(os.path.join(work, "cp_x.sam"), "rb").read(), compresslevel=9, mtime=0))
    shutil.copy(os.path.join(work, "cp_x.contaminants.txt"), os.path.join(HERE, "expected_contam_paired.contaminants.txt"))


def sorted_fixtures(work):
    """`-so` (SortedDataWriter.cpp:186-240, SAMFormat::getSortInfo SAM.cpp:639-685): the SAM records of
    `snap-rna single ... single_reads.fq -t 1 -o out.sam -so` and of `snap-rna paired ...
    contam_paired_{1,2}.fq -t 1 -o out.sam -so` (one sort block each at these sizes)."""
    import gzip
    fa = os.path.join(HERE, "small.fa")
    gidx = os.path.join(work, "gidx")
    ref_index(fa, gidx)
    gtf = os.path.join(HERE, "small.gtf")
    twd = os.path.join(work, "tx")
    os.makedirs(twd, exist_ok=True)
    run([SNAP, "transcriptome", gtf, fa, "tidx", "-O1000"], cwd=twd)
    out = os.path.join(work, "ss.sam")
    run([SNAP, "single", gidx, os.path.join(twd, "tidx"), gtf, os.path.join(HERE, "single_reads.fq"), "-t", "1",
         "-o", out, "-so"], cwd=work)
    with open(out, "rb") as src, open(os.path.join(HERE, "expected_single_sorted.sam.gz"), "wb") as dst:
        dst.write(gzip.compress(src.read(), compresslevel=9, mtime=0))
    out = os.path.join(work, "ps.sam")
    run([SNAP, "paired", gidx, os.path.join(twd, "tidx"), gtf, os.path.join(HERE, "contam_paired_1.fq"),
         os.path.join(HERE, "contam_paired_2.fq"), "-t", "1", "-o", out, "-so"], cwd=work)
    with open(out, "rb") as src, open(os.path.join(HERE, "expected_paired_sorted.sam.gz"), "wb") as dst:
        dst.write(gzip.compress(src.read(), compresslevel=9, mtime=0))


def _rna_blocks_bisect(recs, n, attempt, work, fq0, fq1, stem):
    """Block partition for the RNA fixtures whose every block is a clean `snap-rna paired` run in
    BOTH modes (default and -M), the very runs whose outputs are kept.  The reference's crash in
    AnalyzeReadIntervals depends on heap layout (it can come and go with an output file name), so
    a block is accepted only from its final runs; a failing block is halved, and a single pair
    that still fails is left out.  The block sizes go to expected_<stem>_blocks.json (the test
    aligns the same blocks with fresh GTF counters)."""
    import gzip

    def run_block(idx):
        got = {}
        for tag, extra in (("", []), ("_M", ["-M"])):
            if not attempt(idx, work, extra, out=f"blk{tag}"):
                return None
            lines = open(os.path.join(work, f"blk{tag}.sam")).read().splitlines(keepends=True)
            if sum(1 for l in lines if not l.startswith("@")) != 2 * len(idx):
                return None
            cnt = {cf: open(os.path.join(work, f"blk{tag}.{cf}.counts.txt")).read() for cf in COUNT_FILES}
            got[tag] = (lines, cnt)
        return got

    blocks, drop = [], []

    def solve(idx):
        r = run_block(idx)
        if r is not None:
            blocks.append((idx, r))
        elif len(idx) == 1:
            drop.append(idx[0])
        else:
            h = len(idx) // 2
            solve(idx[:h])
            solve(idx[h:])

    for c in range(0, n, RNA_BLOCK):
        solve(list(range(c, min(n, c + RNA_BLOCK))))
    keep = [i for idx, _ in blocks for i in idx]
    assert keep == sorted(keep)
    for k, x in enumerate((fq0, fq1)):
        with open(x, "w") as f:
            f.write("".join("\n".join(recs[k][4 * i:4 * i + 4]) + "\n" for i in keep))
    if drop:
        print("pairs left out (the reference crashes in AnalyzeReadIntervals):", drop)
    with open(os.path.join(HERE, f"expected_{stem}_blocks.json"), "w") as f:
        json.dump({"block_sizes": [len(idx) for idx, _ in blocks], "dropped_pairs": drop,
                   "note": "blocks of the kept pairs, in order; each block is one reference run"}, f)
    for tag in ("", "_M"):
        body, counts = [], []
        for bi, (idx, r) in enumerate(blocks):
            lines, cnt = r[tag]
            if bi == 0:
                body += [l for l in lines if l.startswith("@")]
            body += [l for l in lines if not l.startswith("@")]
            for cf in COUNT_FILES:
                counts.append(f"## block {bi} {cf}\n")
                counts.append(cnt[cf])
        with open(os.path.join(HERE, f"expected_{stem}_paired{tag}.sam.gz"), "wb") as dst:
            dst.write(gzip.compress("".join(body).encode(), compresslevel=9, mtime=0))
        if not tag:
            with open(os.path.join(HERE, f"expected_{stem}_paired.counts.txt"), "w") as dst:
                dst.write("".join(counts))


RNA_BENCH_BLOCK = 2000


def rna_bench_digest(work, n_pairs=100_000, jobs=8):
    """Reference output for bench.py's `extras.rna_paired` workload (BASELINE configs[4] shape on
    the C2 genome): the C2 synthetic genome written as FASTA and indexed by `snap-rna index`, the
    2,000-gene synthetic GTF and 100k 2 x 150 pairs of tests/rna_synth.py (deterministic, so the GPU
    box regenerates the same inputs), the transcriptome built by `snap-rna transcriptome`, and
    `snap-rna paired ... -t 1` run over blocks of pairs (halved where the reference crashes at the
    end of a run in AnalyzeReadIntervals; a single pair that still crashes is left out).  Stores
    SHA-256 of the concatenated SAM records (no header) in golden.json["rna_bench"]."""
    from concurrent.futures import ThreadPoolExecutor
    from rna_synth import synth_rna_workload
    gg = snapgpu.Genome.synthetic(**C2["genome"])
    gfa = os.path.join(work, "c2.fa")
    gg.write_fasta(gfa)
    gtf, fq0, fq1, info = synth_rna_workload(gg._h, work, n_pairs=n_pairs)
    gidx = os.path.join(work, "gidx")
    ref_index(gfa, gidx)
    twd = os.path.join(work, "tx")
    os.makedirs(twd, exist_ok=True)
    run([SNAP, "transcriptome", gtf, gfa, "tidx", "-O1000"], cwd=twd)
    recs = [open(x).read().splitlines() for x in (fq0, fq1)]
    n = len(recs[0]) // 4
    assert n == n_pairs

    def attempt(idx):
        d = tempfile.mkdtemp(dir=work, prefix="blk")
        try:
            for k in range(2):
                with open(os.path.join(d, f"r_{k}.fq"), "w") as f:
                    f.write("".join("\n".join(recs[k][4 * i:4 * i + 4]) + "\n" for i in idx))
            r = subprocess.run([SNAP, "paired", gidx, os.path.join(twd, "tidx"), gtf, os.path.join(d, "r_0.fq"),
                                os.path.join(d, "r_1.fq"), "-t", "1", "-o", os.path.join(d, "out.sam")],
                               capture_output=True, cwd=d)
            if r.returncode != 0:
                return None
            lines = [l for l in open(os.path.join(d, "out.sam")).read().splitlines(keepends=True)
                     if not l.startswith("@")]
            return lines if len(lines) == 2 * len(idx) else None
        finally:
            shutil.rmtree(d, ignore_errors=True)

    def solve(idx):
        got = attempt(idx)
        if got is not None:
            return [(idx[0], got)], []
        if len(idx) == 1:
            return [], [idx[0]]
        h = len(idx) // 2
        a, da = solve(idx[:h])
        b, db = solve(idx[h:])
        return a + b, da + db

    with ThreadPoolExecutor(jobs) as ex:
        parts = list(ex.map(solve, [list(range(c, min(n, c + RNA_BENCH_BLOCK)))
                                    for c in range(0, n, RNA_BENCH_BLOCK)]))
    blocks = sorted(b for p, _ in parts for b in p)
    drop = sorted(x for _, d in parts for x in d)
    h = hashlib.sha256()
    nrec = 0
    for _, lines in blocks:
        for l in lines:
            h.update(l.encode())
            nrec += 1
    out = {"sha256": h.hexdigest(), "records": nrec, "pairs": n, "dropped_pairs": drop,
           "reference_runs": len(blocks), "workload": info,
           "what": "SHA-256 of the SAM records (header lines excluded) of `snap-rna paired <C2 index> "
                   "<transcriptome> synth.gtf r1 r2 -t 1` over tests/rna_synth.py's 100k 2x150 pairs on the "
                   "C2 genome, in pair order; dropped pairs excluded"}
    gj = os.path.join(HERE, "golden.json")
    meta = json.load(open(gj))
    meta["rna_bench"] = out
    with open(gj, "w") as f:
        json.dump(meta, f, indent=1)
    return out


SINGLE_BENCH_BLOCK = 20000
SINGLE_STATS = r"\t(\d+)\t(\d+) \(at: (\d+)\)"   # AlignerContext::printStats (AlignerContext.cpp:372-393)


def single_bench_reads(work, n_reads=1_000_000):
    """bench.py's `extras.single_e2e` inputs: the C2 genome and tests/rna_synth.py's workload with
    n_reads 100-bp fragments -- the same 2,000-gene GTF as the RNA paired leg (the genes are drawn
    before the reads) -- whose first ends are the single-end reads."""
    from rna_synth import synth_single_reads
    gg = snapgpu.Genome.synthetic(**C2["genome"])
    gtf, fq, info = synth_single_reads(gg._h, work, n_reads)
    return gg, gtf, fq, info


def single_bench_digest(work, n_reads=1_000_000, jobs=8):
    """Reference output and CPU baseline for bench.py's `extras.single_e2e` (`snap-rna single`, SURVEY
    8(f) f1, on the C2 genome): the C2 genome indexed by `snap-rna index`, the transcriptome by `snap-rna
    transcriptome`, and `snap-rna single <gidx> <tidx> synth.gtf reads.fq -t 1` over blocks of reads
    (halved where a run crashes; a read that still crashes alone is left out).  Stores SHA-256 of the
    concatenated SAM records (no header) in golden.json["single_bench"], and the reference's own
    Reads/s (its stats line, alignment time without index load) on a bounded sample: -t 1 and -t 8 with
    BaseAligner.cpp at clang -O3 -fno-strict-return (snap-rna-O3c, oracle/Makefile.ref rna-variants;
    records checked equal to the -O0 build's on the sample)."""
    import re
    from concurrent.futures import ThreadPoolExecutor
    gg, gtf, fq, info = single_bench_reads(work, n_reads)
    gfa = os.path.join(work, "c2.fa")
    gg.write_fasta(gfa)
    gidx = os.path.join(work, "gidx")
    ref_index(gfa, gidx)
    twd = os.path.join(work, "tx")
    os.makedirs(twd, exist_ok=True)
    run([SNAP, "transcriptome", gtf, gfa, "tidx", "-O1000"], cwd=twd)
    recs = open(fq).read().splitlines()
    n = len(recs) // 4
    assert n == n_reads

    def attempt(idx, binary=SNAP, threads=1, timed=False):
        d = tempfile.mkdtemp(dir=work, prefix="blk")
        try:
            with open(os.path.join(d, "r.fq"), "w") as f:
                f.write("".join("\n".join(recs[4 * i:4 * i + 4]) + "\n" for i in idx))
            r = subprocess.run([binary, "single", gidx, os.path.join(twd, "tidx"), gtf, os.path.join(d, "r.fq"),
                                "-t", str(threads), "-o", os.path.join(d, "out.sam")], capture_output=True, text=True,
                               cwd=d)
            if r.returncode != 0:
                return None
            lines = [l for l in open(os.path.join(d, "out.sam")).read().splitlines(keepends=True)
                     if not l.startswith("@")]
            if len(lines) != len(idx):
                return None
            if timed:
                m = re.search(SINGLE_STATS, r.stdout)
                return lines, (int(m.group(1)), int(m.group(2)), int(m.group(3))) if m else None
            return lines
        finally:
            shutil.rmtree(d, ignore_errors=True)

    def solve(idx):
        got = attempt(idx)
        if got is not None:
            return [(idx[0], got)], []
        if len(idx) == 1:
            return [], [idx[0]]
        h = len(idx) // 2
        a, da = solve(idx[:h])
        b, db = solve(idx[h:])
        return a + b, da + db

    with ThreadPoolExecutor(jobs) as ex:
        parts = list(ex.map(solve, [list(range(c, min(n, c + SINGLE_BENCH_BLOCK)))
                                    for c in range(0, n, SINGLE_BENCH_BLOCK)]))
    blocks = sorted(b for p, _ in parts for b in p)
    drop = sorted(x for _, d in parts for x in d)
    by_first = dict(blocks)
    h = hashlib.sha256()
    nrec = 0
    for _, lines in blocks:
        for l in lines:
            h.update(l.encode())
            nrec += 1
    # CPU baseline: the reference CLI's own rate on a bounded sample, one block at a time (no other load)
    snap_o3c = SNAP + "-O3c"
    cpu = {}
    for threads, nblk, blk in ((1, 3, SINGLE_BENCH_BLOCK), (8, 2, 5 * SINGLE_BENCH_BLOCK)):
        runs, same = [], True
        for b in range(nblk):
            first = b * (n // nblk) // SINGLE_BENCH_BLOCK * SINGLE_BENCH_BLOCK   # on the digest's block grid
            idx = list(range(first, min(n, first + blk)))
            got = attempt(idx, snap_o3c, threads, timed=True)
            if got is None or got[1] is None:
                continue
            lines, (tot, rps, ms) = got
            runs.append({"first_read": first, "reads": tot, "reads_per_s_printed": rps, "align_ms": ms})
            if threads == 1:   # the -O0 build's records on the same reads (the digest's blocks)
                ref = [l for f0 in range(first, first + blk, SINGLE_BENCH_BLOCK) for l in by_first.get(f0, [])]
                same = same and ref == lines
        reads = sum(r["reads"] for r in runs)
        ms = sum(r["align_ms"] for r in runs)
        cpu[f"threads_{threads}"] = {
            "value": reads / (ms / 1000.0) if ms else None, "unit": "reads/s", "cores": threads,
            "kind": "reference, build container", "base_aligner_opt": "-O3c",
            "sample": f"{reads} of the {n} reads ({len(runs)} blocks of {blk}, spread over the set), `snap-rna "
                      f"single <C2 index> <transcriptome> synth.gtf reads.fq -t {threads}` with BaseAligner.cpp at "
                      "clang -O3 -fno-strict-return (oracle/Makefile.ref rna-variants); time = the reference's own "
                      "alignment time (AlignerContext::printStats), index load excluded",
            "blocks": runs, "host": {"nproc": os.cpu_count()}}
        if threads == 1:
            cpu["threads_1"]["records_equal_to_O0"] = same
    out = {"sha256": h.hexdigest(), "records": nrec, "reads": n, "dropped_reads": drop,
           "reference_runs": len(blocks), "workload": info, "cpu_baseline": cpu,
           "what": "SHA-256 of the SAM records (header lines excluded) of `snap-rna single <C2 index> "
                   "<transcriptome> synth.gtf reads.fq -t 1` over the first ends of tests/rna_synth.py's "
                   f"{n} 100-bp fragments on the C2 genome, in read order; dropped reads excluded"}
    gj = os.path.join(HERE, "golden.json")
    meta = json.load(open(gj))
    meta["single_bench"] = out
    with open(gj, "w") as f:
        json.dump(meta, f, indent=1)
    return out


def _bam_unpack(raw):
    """-> (reference list [[name, l_ref]], record bytes) of a decompressed BAM stream."""
    import struct
    assert raw[:4] == b"BAM\1"
    at = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", raw, at)[0]
        refs.append([raw[at + 4:at + 4 + ln - 1].decode(), struct.unpack_from("<i", raw, at + 4 + ln)[0]])
        at += 8 + ln
    return refs, raw[at:]


def _bam_count(recs):
    import struct
    n, at = 0, 0
    while at < len(recs):
        at += 4 + struct.unpack_from("<i", recs, at)[0]
        n += 1
    return n


def rna_bam_fixtures(work):
    """`snap-rna paired ... -o out.bam` (SimpleReadWriter::writePair -> BAMFormat::writeRead with the
    mate, ReadWriter.cpp:133-217, Bam.cpp:596-790) over the same blocks as the SAM fixtures of both
    RNA read sets (2 x <=101 in blocks of 200, 2 x 150 over expected_rna150_blocks.json).  A block
    whose run exits non-zero is kept when its BGZF stream is complete (EOF block) and holds both
    records of every pair: the reference writes and closes the BAM before the crash in
    AnalyzeReadIntervals that comes and goes with heap layout.  Stores the decompressed records of
    the blocks concatenated and the reference list."""
    import gzip
    fa = os.path.join(HERE, "small.fa")
    gtf = os.path.join(HERE, "small.gtf")
    gidx = os.path.join(work, "gidx")
    ref_index(fa, gidx)
    twd = os.path.join(work, "tx")
    os.makedirs(twd, exist_ok=True)
    run([SNAP, "transcriptome", gtf, fa, "tidx", "-O1000"], cwd=twd)
    eof = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    for stem in ("rna", "rna150"):
        recs = [open(os.path.join(HERE, f"{stem}_{k}.fq")).read().splitlines() for k in (1, 2)]
        n = len(recs[0]) // 4
        bj = os.path.join(HERE, f"expected_{stem}_blocks.json")
        sizes = json.load(open(bj))["block_sizes"] if os.path.exists(bj) else \
            [min(RNA_BLOCK, n - c) for c in range(0, n, RNA_BLOCK)]
        for tag, extra in (("", []), ("_M", ["-M"])):
            body, refs, at = [], None, 0
            for sz in sizes:
                for k in range(2):
                    with open(os.path.join(work, f"b_{k}.fq"), "w") as f:
                        f.write("".join("\n".join(recs[k][4 * i:4 * i + 4]) + "\n" for i in range(at, at + sz)))
                out = os.path.join(work, "b.bam")
                if os.path.exists(out):
                    os.unlink(out)
                subprocess.run([SNAP, "paired", gidx, os.path.join(twd, "tidx"), gtf, os.path.join(work, "b_0.fq"),
                                os.path.join(work, "b_1.fq"), "-t", "1", "-o", out] + extra, capture_output=True,
                               cwd=work)
                data = open(out, "rb").read()
                assert data.endswith(eof), f"{stem} block at {at}: incomplete BAM"
                rf, rc_ = _bam_unpack(gzip.decompress(data))
                assert _bam_count(rc_) == 2 * sz, f"{stem} block at {at}: {_bam_count(rc_)} records"
                refs = refs or rf
                body.append(rc_)
                at += sz
            with open(os.path.join(HERE, f"expected_{stem}_paired{tag}.bam.records.gz"), "wb") as f:
                f.write(gzip.compress(b"".join(body), compresslevel=9, mtime=0))
            with open(os.path.join(HERE, f"expected_{stem}_paired.bam.refs.json"), "w") as f:
                json.dump(refs, f)


def long_fixtures(work):
    """Reads of 129..256 bases (align_kernel<256>: 256-bit bit-plane masks) on the small genome:
    synthetic 150 / 250 bp and mixed-length reads with the reference's own AlignRead outputs for
    three parameter sets, and Landau-Vishkin vectors with patterns of 128..253 bases."""
    fa = os.path.join(HERE, "small.fa")
    g = snapgpu.Genome.from_fasta(fa, 500)
    rd = []
    for rl, cnt, seed in ((150, 1200, 41), (250, 600, 42), (129, 150, 43), (256, 150, 44)):
        syn = snapgpu.Reads.synthetic(g, cnt, seed=seed, read_length=rl, random_read_fraction=0.02)
        rd += [tuple(x.decode() for x in syn.get(i)) for i in range(syn.n)]
    rng = random.Random(45)
    syn = snapgpu.Reads.synthetic(g, 400, seed=46, read_length=256, random_read_fraction=0.02)
    for i in range(syn.n):   # mixed lengths 129..256, some lower-case and N bases
        b, q = (x.decode() for x in syn.get(i))
        L = rng.randrange(129, 257)
        b, q = list(b[:L]), q[:L]
        for _ in range(rng.randrange(0, 3)):
            b[rng.randrange(L)] = "N"
        b = "".join(b)
        if rng.random() < 0.1:
            b = b.lower()
        rd.append((b, q))
    fq = os.path.join(HERE, "small_long_reads.fq")
    write_fastq(fq, rd)
    idxdir = os.path.join(work, "small_idx_long")
    ref_index(fa, idxdir)
    for name in ("default", "k20", "s4"):
        with open(os.path.join(HERE, f"expected_small_long_{name}.tsv"), "w") as f:
            f.write(ref_align(idxdir, fq, PARAM_SETS[name]))
    for direction in (1, -1):
        rows = []
        for _ in range(400):
            L = rng.choice([128, 140, 160, 190, 220, 240, 253])
            t = "".join(rng.choice("ACGT") for _ in range(L + 35))
            p = list(t[:L] if direction > 0 else t[::-1][:L])
            for _ in range(rng.randrange(0, 12)):
                op, i = rng.random(), rng.randrange(len(p))
                if op < 0.6:
                    p[i] = rng.choice("ACGTN")
                elif op < 0.8 and len(p) < 253:
                    p.insert(i, rng.choice("ACGT"))
                elif len(p) > 128:
                    del p[i]
            p = "".join(p)
            q = "".join(chr(33 + rng.randrange(0, 45)) for _ in p)
            k = rng.choice([0, 1, 2, 3, 5, 8, 14, 16, 22, 30])
            tl = rng.choice([len(t), len(p) + 31])
            tt = t[:tl] if direction > 0 else t[-tl:]
            rows.append((direction, k, tt, p, q))
        inp = os.path.join(work, f"lvl{direction}.tsv")
        with open(inp, "w") as f:
            for r in rows:
                f.write("\t".join(map(str, r)) + "\n")
        out = run([HARNESS, "lv", inp]).splitlines()
        with open(os.path.join(HERE, f"lv_long_{'fwd' if direction > 0 else 'rev'}.tsv"), "w") as f:
            for r, o in zip(rows, out):
                e, net, prob = o.split("\t")
                f.write("\t".join(map(str, r)) + f"\t{e}\t{net}\t{float.fromhex(prob).hex()}\n")


def bam_fixtures(work):
    """`snap-rna single <genome> <transcriptome> <gtf> single_reads.fq -t 1 -o out.bam` (BAMFormat::
    writeHeader / writeRead, Bam.cpp:542-790): the BGZF stream decompressed, split into the header's
    reference list and the alignment records (the header text echoes the command line)."""
    import gzip
    import struct
    fa = os.path.join(HERE, "small.fa")
    gtf = os.path.join(HERE, "small.gtf")
    fq = os.path.join(HERE, "single_reads.fq")
    gidx = os.path.join(work, "gidx")
    ref_index(fa, gidx)
    twd = os.path.join(work, "tx")
    os.makedirs(twd, exist_ok=True)
    run([SNAP, "transcriptome", gtf, fa, "tidx", "-O1000"], cwd=twd)
    for tag, extra in (("", []), ("_M", ["-M"])):
        out = os.path.join(work, f"out{tag}.bam")
        run([SNAP, "single", gidx, os.path.join(twd, "tidx"), gtf, fq, "-t", "1", "-o", out] + extra, cwd=work)
        raw = gzip.decompress(open(out, "rb").read())
        assert raw[:4] == b"BAM\1"
        l_text = struct.unpack_from("<i", raw, 4)[0]
        at = 8 + l_text
        n_ref = struct.unpack_from("<i", raw, at)[0]
        at += 4
        refs = []
        for _ in range(n_ref):
            ln = struct.unpack_from("<i", raw, at)[0]
            name = raw[at + 4:at + 4 + ln - 1].decode()
            lref = struct.unpack_from("<i", raw, at + 4 + ln)[0]
            refs.append([name, lref])
            at += 8 + ln
        with open(os.path.join(HERE, f"expected_single{tag}.bam.refs.json"), "w") as f:
            json.dump(refs, f)
        with open(os.path.join(HERE, f"expected_single{tag}.bam.records.gz"), "wb") as f:
            f.write(gzip.compress(raw[at:], compresslevel=9, mtime=0))


def rna_fs_fixtures(work):
    """`snap-rna paired ... -fs` (PairedAligner.cpp:274-275, 648-651: a pair with exactly one end
    SingleHit becomes NotFound on both ends) on the 2 x <=101 RNA set, in the same blocks of
    RNA_BLOCK pairs as expected_rna_paired.sam.gz: the SAM records only."""
    import gzip
    fa, gtf = os.path.join(HERE, "small.fa"), os.path.join(HERE, "small.gtf")
    fq = [os.path.join(HERE, f"rna_{k}.fq") for k in (1, 2)]
    gidx = os.path.join(work, "gidx")
    ref_index(fa, gidx)
    twd = os.path.join(work, "tx")
    os.makedirs(twd, exist_ok=True)
    run([SNAP, "transcriptome", gtf, fa, "tidx", "-O1000"], cwd=twd)
    recs = [open(x).read().splitlines() for x in fq]
    n = len(recs[0]) // 4
    # With -fs the reference segfaults before writing any record in most blocks (SIGSEGV, empty SAM:
    # a crash of its own, not restated); the blocks it completes are the fixture, their starts kept
    # in expected_rna_paired_fs_blocks.json.
    body, starts, plain_differs = [], [], 0
    for c in range(0, n, RNA_BLOCK):
        for k in range(2):
            with open(os.path.join(work, f"fs_{k}.fq"), "w") as f:
                f.write("".join("\n".join(recs[k][4 * i:4 * i + 4]) + "\n" for i in range(c, min(n, c + RNA_BLOCK))))
        outs = {}
        for tag, extra in (("fs", ["-fs"]), ("plain", [])):
            r = subprocess.run([SNAP, "paired", gidx, os.path.join(twd, "tidx"), gtf, os.path.join(work, "fs_0.fq"),
                                os.path.join(work, "fs_1.fq"), "-t", "1", "-o", os.path.join(work, f"{tag}.sam")] + extra,
                               capture_output=True, cwd=work)
            outs[tag] = open(os.path.join(work, f"{tag}.sam")).read().splitlines(keepends=True) if r.returncode == 0 else None
        if outs["fs"] is None:
            continue
        if not starts:
            body += [l for l in outs["fs"] if l.startswith("@")]
        recs_fs = [l for l in outs["fs"] if not l.startswith("@")]
        body += recs_fs
        plain_differs += sum(1 for a, b in zip(recs_fs, [l for l in outs["plain"] if not l.startswith("@")]) if a != b)
        starts.append(c)
    with open(os.path.join(HERE, "expected_rna_paired_fs.sam.gz"), "wb") as dst:
        dst.write(gzip.compress("".join(body).encode(), compresslevel=9, mtime=0))
    with open(os.path.join(HERE, "expected_rna_paired_fs_blocks.json"), "w") as dst:
        json.dump({"block": RNA_BLOCK, "starts": starts, "records_differing_from_plain": plain_differs}, dst)


EDGE_LENGTHS = (49, 50, 64, 128, 129, 192, 193, 256, 257, 320, 384, 448, 499, 500)
_COMP = str.maketrans("ACGTN", "TGCAN")


def _rc(x):
    return x.translate(_COMP)[::-1]


def _fasta_seqs(fa):
    """contig name -> upper-cased sequence (IUPAC bytes kept, as FASTA.cpp:104-116 keeps them)."""
    seqs, name = {}, None
    for line in open(fa):
        line = line.strip()
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(line.upper())
    return {k: "".join(v) for k, v in seqs.items()}


def _keep_gz(name, text):
    """A fixture kept gzipped (tests/golden/<name>.gz; golden_common.golden_path unpacks it for the tests);
    mtime 0: reproducible bytes."""
    import gzip
    with open(os.path.join(HERE, name + ".gz"), "wb") as f:
        f.write(gzip.compress(text.encode(), compresslevel=9, mtime=0))


def _write_pairs(work, stem, pairs, tag):
    """<stem>_{1,2}.fq in `work` for the reference, gzipped into tests/golden."""
    for k in (0, 1):
        text = "".join(f"@{tag}{i}/{k + 1}\n{p[2 * k]}\n+\n{p[2 * k + 1]}\n" for i, p in enumerate(pairs))
        with open(os.path.join(work, f"{stem}_{k + 1}.fq"), "w") as f:
            f.write(text)
        _keep_gz(f"{stem}_{k + 1}.fq", text)


def _edge_mutate(s, rng):
    """Substitutions and indels that scale with the length (scores span 0..maxK at every length); the
    length is kept (an insertion drops the tail, a deletion appends random bases), so a 500-base mate
    stays within the reference's MAX_READ_LENGTH."""
    L, scale = len(s), 1 + len(s) // 128
    s = list(s)
    for _ in range(rng.choice([0, 0, 0, 1, 1, 2, 3, 5]) * scale):
        s[rng.randrange(L)] = rng.choice("ACGT")
    for _ in range(scale):
        if rng.random() < 0.06 and L > 20:
            j = rng.randrange(5, L - 5)
            s = s[:j] + s[j + rng.randrange(1, 4):] if rng.random() < 0.5 else s[:j] + list("TGA"[:rng.randrange(1, 4)]) + s[j:]
    s = s[:L] + [rng.choice("ACGT") for _ in range(L - len(s))]
    return "".join(s)


def paired_edge_long_reads(seqs, rng, n_pairs=360):
    """The `long` pairs: paired_reads' mix (proper, overlapping, past maxSpacing, chimeric, one or both
    mates random, N-rich, same-orientation) with each mate's length drawn on its own from EDGE_LENGTHS,
    plus pairs laid over one of the genome's IUPAC bytes (forward strand, so the read carries the same
    byte) and pairs within 500 bases of a contig's start or end.  -> (pairs, counts)."""
    names = list(seqs)
    iupac = [(c, i) for c in names for i, ch in enumerate(seqs[c]) if ch not in "ACGTN"]
    counts = dict(end_lo=0, end_hi=0)

    def rand_seq(L):
        return "".join(rng.choice("ACGT") for _ in range(L))

    def frag_at(c, pos, L0, L1, ins, flip):
        f = seqs[c][pos:pos + ins]
        assert len(f) == ins >= max(L0, L1)
        if flip:
            f = _rc(f)
        return f[:L0], _rc(f[len(f) - L1:])

    def frag_pair(L0, L1, ins):
        c = rng.choice(names)
        ins = max(ins, L0, L1)
        return frag_at(c, rng.randrange(0, len(seqs[c]) - ins), L0, L1, ins, rng.random() < 0.5)

    pairs = []
    for i in range(n_pairs):
        u = rng.random()
        L0, L1 = rng.choice(EDGE_LENGTHS), rng.choice(EDGE_LENGTHS)
        M = max(L0, L1)
        if u < 0.44:
            a, b = frag_pair(L0, L1, M + rng.randrange(0, 550))
        elif u < 0.49:
            a, b = frag_pair(L0, L1, M + rng.randrange(0, 40))               # mates overlap: within minSpacing
        elif u < 0.53:
            a, b = frag_pair(L0, L1, M + rng.randrange(1100, 4000))          # beyond maxSpacing
        elif u < 0.60:
            a, _ = frag_pair(L0, L1, M + 300)                                # chimeric
            _, b = frag_pair(L0, L1, M + 300)
        elif u < 0.65:
            a, b = frag_pair(L0, L1, M + 300)
            if rng.random() < 0.5:
                a = rand_seq(L0)
            else:
                b = rand_seq(L1)
        elif u < 0.70:
            a, b = rand_seq(L0), rand_seq(L1)
        elif u < 0.74:
            a, b = frag_pair(L0, L1, M + 300)
            a = "".join("N" if rng.random() < 0.08 else ch for ch in a)      # N-rich (> maxK Ns once long enough)
        elif u < 0.78:
            a, b = frag_pair(L0, L1, M + 300)
            b = _rc(b)                                                       # same orientation
        elif u < 0.90:   # over an IUPAC byte of the genome; half of them with both mates of 50..256 bases
            if rng.random() < 0.5:
                L0, L1 = (rng.choice([x for x in EDGE_LENGTHS if 50 <= x <= 256]) for _ in range(2))
                M = max(L0, L1)
            c, at = rng.choice(iupac)
            ins = M + rng.randrange(0, 400)
            pos = min(max(0, at - rng.randrange(0, L0)), len(seqs[c]) - ins)
            a, b = frag_at(c, pos, L0, L1, ins, False)
        else:            # within 500 bases of a contig's start / end
            c = rng.choice(names)
            ins = M + rng.randrange(0, 400)
            lo = rng.random() < 0.5
            pos = rng.randrange(0, 400) if lo else len(seqs[c]) - ins - rng.randrange(0, 400)
            counts["end_lo" if lo else "end_hi"] += 1
            a, b = frag_at(c, pos, L0, L1, ins, rng.random() < 0.5)
        if rng.random() < 0.5:
            a, b = b, a
        a, b = _edge_mutate(a, rng), _edge_mutate(b, rng)
        if rng.random() < 0.05:
            a = a.lower()
        qa, qb = ["I"] * len(a), ["I"] * len(b)
        if rng.random() < 0.1:
            qa = [rng.choice("#+5?I") for _ in a]
        pairs.append((a, "".join(qa), b, "".join(qb)))
    return pairs, counts


def _edge_long_asserts(pairs, counts):
    """The length classes and edge counts the `long` set promises, from the FASTQ text alone."""
    L = [(len(a), len(b)) for a, _, b, _ in pairs]
    mx = [max(x) for x in L]
    assert sum(1 for m in mx if m <= 128) >= 20 and sum(1 for m in mx if 129 <= m <= 256) >= 20
    assert sum(1 for m in mx if m >= 257) >= 20
    assert sum(1 for x in L if min(x) <= 128 and max(x) > 256) >= 20
    assert sum(1 for x in L if 500 in x) >= 10 and sum(1 for x in L if 49 in x) >= 10
    assert sum(1 for x in L if x[0] != x[1] and min(x) >= 50) >= 200
    assert sum(1 for x in L if max(x) < 50) >= 1                  # both mates short: written by no pass
    other = lambda s: bool(set(s.upper()) - set("ACGTN"))
    n_iupac = sum(1 for a, _, b, _ in pairs if other(a) or other(b))
    assert n_iupac >= 15, n_iupac
    # the routing rule for IUPAC pairs needs some with both mates of 50..256 bases
    assert sum(1 for a, _, b, _ in pairs if (other(a) or other(b)) and 50 <= min(len(a), len(b)) and
               max(len(a), len(b)) <= 256) >= 5
    assert counts["end_lo"] >= 5 and counts["end_hi"] >= 5, counts


def _ref_paired(idx, fq0, fq1, p):
    args = [str(p[k]) for k in ("maxHits", "maxK", "numSeeds", "extra", "minSpacing", "maxSpacing", "maxBigHits")]
    if "seedCoverage" in p:
        args.append(repr(p["seedCoverage"]))
    return run([HARNESS, "paired", idx, fq0, fq1] + args)


def tandem_genome_and_pairs(rng):
    """tandem.fa: one contig of random sequence holding one array of 300 copies of a 20-base unit, each
    copy with 0..2 substitutions; 100-base mates inside the array, across its borders and in the flanks.
    -> (sequence, pairs, per pair the larger count of a mate's first seed, either strand, within 3000
    bases of the other mate)."""
    flank, n_copies = 40000, 300
    unit = "".join(rng.choice("ACGT") for _ in range(20))
    copies = []
    for _ in range(n_copies):
        c = list(unit)
        for _ in range(rng.choice([0, 0, 0, 0, 1, 2])):
            j = rng.randrange(20)
            c[j] = rng.choice([x for x in "ACGT" if x != c[j]])
        copies.append("".join(c))
    g = "".join(rng.choice("ACGT") for _ in range(flank)) + "".join(copies) + \
        "".join(rng.choice("ACGT") for _ in range(flank))
    A, B = flank, flank + 20 * n_copies

    def count(seed, lo, hi):
        w, n = g[max(0, lo):hi], 0
        for s in {seed, _rc(seed)}:
            at = w.find(s)
            while at >= 0:
                n += 1
                at = w.find(s, at + 1)
        return n

    pairs, seen = [], []
    for i in range(80):
        if i < 40:      # both mates inside the array
            ins = rng.randrange(150, 2900)
            pos = rng.randrange(A, B - ins)
        elif i < 68:    # one mate inside, one in a flank (up to maxSpacing away)
            ins = rng.randrange(250, 2900)
            pos = rng.randrange(A - ins + 100, A - 100 + 1) if i % 2 else rng.randrange(B - ins + 100, B - 100 + 1)
        else:           # both in a flank
            ins = rng.randrange(150, 700)
            pos = rng.randrange(1000, A - 3000) if i % 2 else rng.randrange(B + 3000, len(g) - 1000)
        f = g[pos:pos + ins]
        flip = rng.random() < 0.5
        pa, pb = (pos, pos + ins - 100)
        a, b = f[:100], _rc(f[-100:])
        if flip:
            a, b, pa, pb = b, a, pb, pa
        # the first seed of each mate as the genome holds it (the reads are mutated afterwards)
        seen.append(max(count(a[:20], pb - 3000, pb + 3100), count(b[:20], pa - 3000, pa + 3100)))
        mut = []
        for s in (a, b):
            s = list(s)
            for _ in range(rng.choice([0, 0, 1, 2, 3])):
                s[rng.randrange(20, 100)] = rng.choice("ACGT")
            mut.append("".join(s))
        pairs.append((mut[0], "I" * 100, mut[1], "I" * 100))
    return g, pairs, seen


def repeat_pairs(seqs, rng, n_pairs=120):
    """Pairs of 100-base mates on repeat.fa (contigs: a 5,000-base random head, then 600 copies of a
    150-base element 20..60 bases apart): both mates inside copies, or one inside a copy and one in the
    head; inserts of 150..700."""
    erng = random.Random(77)                                   # the element multihit_alias_fixtures drew
    elem = "".join(erng.choice("ACGT") for _ in range(150))
    starts = {}
    for c, g in seqs.items():
        st = []
        for key, off in ((elem[:40], 0), (_rc(elem)[-40:], 110)):   # substitutions sit at 40, 75, 110 only
            at = g.find(key)
            while at >= 0:
                st.append(at - off)
                at = g.find(key, at + 1)
        starts[c] = sorted(x for x in st if x >= 5000)
        assert len(starts[c]) == 600, (c, len(starts[c]))
    pairs = []
    for i in range(n_pairs):
        c = rng.choice(list(seqs))
        g, st = seqs[c], starts[c]
        if i % 3 < 2:   # both mates inside copies
            while True:
                j = rng.randrange(len(st))
                k = rng.randrange(j, min(len(st), j + 4))
                s, e = st[j] + rng.randrange(0, 50), st[k] + rng.randrange(100, 151)
                if 150 <= e - s <= 700:
                    break
        else:           # one mate in the random head, its mate inside one of the first copies
            while True:
                e = st[rng.randrange(0, 3)] + rng.randrange(100, 151)
                s = e - rng.randrange(150, 701)
                if s + 100 <= 5000:
                    break
        f = g[s:e]
        a, b = f[:100], _rc(f[-100:])
        if rng.random() < 0.5:
            a, b = b, a
        mut = []
        for x in (a, b):
            x = list(x)
            for _ in range(rng.choice([0, 0, 1, 2, 4])):
                x[rng.randrange(100)] = rng.choice("ACGT")
            mut.append("".join(x))
        pairs.append((mut[0], "I" * 100, mut[1], "I" * 100))
    return pairs


def paired_edge_fixtures(work):
    """The PAIRED_EDGE_SETS of golden_common.py (tests/test_paired_edges.py): reads of 257..500 bases
    and mates of different lengths (`long`), more than 64 mates inside one spacing window (`tandem`),
    pairs on the 1,800-copy repeat genome (`repeat`), seed lengths 16 and 25, and the seedCoverage seed
    count (`coverage`), each through `ref_harness paired`.  Every promise the sets make (length classes,
    IUPAC and contig-end pairs, outcome mix, seed occurrence counts, maxBigHits biting) is asserted here."""
    from golden_common import PAIRED_EDGE_SETS, PAIRED_EDGE_FIRST, PAIRED_EDGE_MAXLEN
    # --- the new inputs (kept gzipped: the `long` mates alone are 375 KB of text)
    small = _fasta_seqs(os.path.join(HERE, "small.fa"))
    pairs, counts = paired_edge_long_reads(small, random.Random(257))
    _edge_long_asserts(pairs, counts)
    _write_pairs(work, "paired_edge_long", pairs, "el")
    # coverage: the long pairs with both mates <= 256 bases: at seedCoverage 2.0 none asks for more seeds
    # than the reference's MAX_MAX_SEEDS (30, IntersectingPairedEndAligner.h:93: its lookup arrays)
    cov = [p for p in pairs if max(len(p[0]), len(p[2])) <= PAIRED_EDGE_MAXLEN["coverage"]]
    cp = PAIRED_EDGE_SETS["coverage"][3]
    assert all(int(max(len(p[0]), len(p[2])) * cp["seedCoverage"] / 20) <= 30 for p in cov) and len(cov) >= 100
    g, tp, seen = tandem_genome_and_pairs(random.Random(307))
    fasta = ">tandem0\n" + "".join(g[i:i + 70] + "\n" for i in range(0, len(g), 70))
    assert len(fasta) < 100_000
    with open(os.path.join(work, "tandem.fa"), "w") as f:
        f.write(fasta)
    _keep_gz("tandem.fa", fasta)
    # the scan for the lowest best-possible score walks the mates 64 per step: > 128 mates in one window
    # make it three steps, 65..128 two
    assert sum(1 for x in seen if x > 128) >= 20 and sum(1 for x in seen if 65 <= x <= 128) >= 10, sorted(seen)
    _write_pairs(work, "paired_edge_tandem", tp, "et")
    _write_pairs(work, "paired_edge_repeat", repeat_pairs(_fasta_seqs(os.path.join(HERE, "repeat.fa")), random.Random(1801)), "er")
    # --- the reference's rows
    idx_of, rows = {}, {}
    for name, (fa, seed_len, stem, p) in PAIRED_EDGE_SETS.items():
        key = (fa, seed_len)
        if key not in idx_of:
            idx_of[key] = os.path.join(work, f"eidx_{fa}_{seed_len}")
            shutil.rmtree(idx_of[key], ignore_errors=True)
            # the dense repeats need the larger overflow space (as multihit_alias_fixtures)
            run([SNAP, "index", os.path.join(work if fa == "tandem.fa" else HERE, fa), idx_of[key], "-s", str(seed_len)] +
                (["-O1000"] if fa != "small.fa" else []))
        # the pairs of the set: all of <stem>_{1,2}.fq, its first pairs, or its pairs of bounded mate length
        recs = [open(os.path.join(work if stem.startswith("paired_edge") else HERE, f"{stem}_{k}.fq")).read().splitlines()
                for k in (1, 2)]
        n = len(recs[0]) // 4
        take = [i for i in range(min(n, PAIRED_EDGE_FIRST.get(name, n)))
                if max(len(recs[0][4 * i + 1]), len(recs[1][4 * i + 1])) <= PAIRED_EDGE_MAXLEN.get(name, 500)]
        if name == "coverage":
            assert len(take) == len(cov)
        fq = [os.path.join(work, f"set_{k}.fq") for k in (1, 2)]
        for k in range(2):
            with open(fq[k], "w") as f:
                f.write("".join("\n".join(recs[k][4 * i:4 * i + 4]) + "\n" for i in take))
        out = _ref_paired(idx_of[key], fq[0], fq[1], p)
        rows[name] = out.splitlines()
        # a pair the reference cannot complete (a soft exit) ends its output early
        assert len(rows[name]) == len(take), f"{name}: the reference wrote {len(rows[name])} rows for {len(take)} pairs"
        _keep_gz(f"expected_paired_edge_{name}.tsv", out)
    chim = [r.split("\t")[12:25] for r in rows["long_default"]]
    together = sum(1 for c in chim if c[10] == "1")
    fallback = sum(1 for c in chim if c[10] == "0" and c[0] != "0")
    untouched = sum(1 for c in chim if c[0] == "0" and c[1] == "0" and c[2] == str(0xFFFFFFFF))
    assert together >= 100 and fallback >= 20 and untouched >= 10, (together, fallback, untouched)
    differ = sum(1 for a, b in zip(rows["repeat_default"], rows["repeat_wide"]) if a != b)
    assert differ >= 20, differ                                  # maxBigHits 64 biting
    print("long/default: together", together, "fallback", fallback, "untouched", untouched,
          "| repeat: wide differs from default on", differ, "pairs | tandem first-seed counts", sorted(seen))


def verylong_fixtures(work):
    """Single-end reads of 257..500 bases (align_kernel<512>, byte compares) on the small genome, built
    as long_fixtures builds its reads: fixed lengths and a mixed-length tail, some lower-case, some with
    N bases, with the reference's AlignRead outputs for three parameter sets."""
    from golden_common import VERYLONG_SETS
    fa = os.path.join(HERE, "small.fa")
    g = snapgpu.Genome.from_fasta(fa, 500)
    rd = []
    for rl, cnt, seed in ((257, 30, 141), (300, 50, 142), (320, 30, 143), (384, 30, 144), (448, 30, 145),
                          (499, 30, 146), (500, 40, 147)):
        syn = snapgpu.Reads.synthetic(g, cnt, seed=seed, read_length=rl, random_read_fraction=0.02)
        rd += [tuple(x.decode() for x in syn.get(i)) for i in range(syn.n)]
    rng = random.Random(148)
    syn = snapgpu.Reads.synthetic(g, 60, seed=149, read_length=500, random_read_fraction=0.02)
    for i in range(syn.n):   # mixed lengths 257..500, some lower-case and N bases
        b, q = (x.decode() for x in syn.get(i))
        L = rng.randrange(257, 501)
        b, q = list(b[:L]), q[:L]
        for _ in range(rng.randrange(0, 3)):
            b[rng.randrange(L)] = "N"
        b = "".join(b)
        if rng.random() < 0.1:
            b = b.lower()
        rd.append((b, q))
    fq = os.path.join(work, "small_verylong_reads.fq")
    write_fastq(fq, rd)
    _keep_gz("small_verylong_reads.fq", open(fq).read())
    idxdir = os.path.join(work, "small_idx_verylong")
    ref_index(fa, idxdir)
    for name in VERYLONG_SETS:
        _keep_gz(f"expected_small_verylong_{name}.tsv", ref_align(idxdir, fq, PARAM_SETS[name]))


def main():
    work = tempfile.mkdtemp(prefix="golden_")
    if "--only-paired-edges" in sys.argv:
        paired_edge_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("paired edge fixtures written to", HERE)
        return
    if "--only-verylong" in sys.argv:
        verylong_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("257..500-base read fixtures written to", HERE)
        return
    if "--only-bam" in sys.argv:
        bam_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("BAM fixtures written to", HERE)
        return
    if "--only-long" in sys.argv:
        long_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("129..256-base read and LV fixtures written to", HERE)
        return
    if "--only-rna-bench" in sys.argv:
        n = int(sys.argv[sys.argv.index("--only-rna-bench") + 1]) if len(sys.argv) > 2 else 100_000
        print(json.dumps({k: v for k, v in rna_bench_digest(work, n).items() if k != "workload"}))
        shutil.rmtree(work, ignore_errors=True)
        return
    if "--only-single-bench" in sys.argv:
        i = sys.argv.index("--only-single-bench")
        n = int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 1_000_000
        print(json.dumps({k: v for k, v in single_bench_digest(work, n).items() if k != "workload"}))
        shutil.rmtree(work, ignore_errors=True)
        return
    if "--only-rna-fs" in sys.argv:
        rna_fs_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("RNA paired -fs fixture written to", HERE)
        return
    if "--only-rna-bam" in sys.argv:
        rna_bam_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("RNA paired BAM fixtures written to", HERE)
        return
    if "--only-sorted" in sys.argv:
        sorted_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("sorted-output fixtures written to", HERE)
        return
    if "--only-contam" in sys.argv:
        contamination_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("contamination-database fixtures written to", HERE)
        return
    if "--only-rna150" in sys.argv:
        rna_paired_fixtures(work, "150")
        shutil.rmtree(work, ignore_errors=True)
        print("2 x 150 RNA paired product path fixtures written to", HERE)
        return
    if "--only-rna-paired" in sys.argv:
        rna_paired_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("RNA paired product path fixtures written to", HERE)
        return
    if "--only-mh1000" in sys.argv:
        multihit_alias_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("maxHitsToGet 1000 fixtures written to", HERE)
        return
    if "--only-charseeds" in sys.argv:
        charseeds_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("CharacterizeSeeds fixtures written to", HERE)
        return
    if "--only-paired" in sys.argv:
        paired_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("paired-end fixtures written to", HERE)
        return
    if "--only-single" in sys.argv:
        single_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("single-end product path fixtures written to", HERE)
        return
    if "--only-refindex" in sys.argv:
        refindex_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("reference index + seedLen fixtures written to", HERE)
        return
    if "--only-cigar" in sys.argv:
        cigar_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("CIGAR / SAM fixtures written to", HERE)
        return
    if "--only-multihit" in sys.argv:
        multihit_fixtures(work)
        shutil.rmtree(work, ignore_errors=True)
        print("multi-hit fixtures written to", HERE)
        return
    meta = {"generator": "tests/golden/make_golden.py", "reference": "oracle/_ref (andrewmagis/snap-rna SNAPLib)"}

    # 1. small genome + edge/synthetic reads, several parameter sets
    fa = os.path.join(HERE, "small.fa")
    small_genome_fasta(fa)
    g = snapgpu.Genome.from_fasta(fa, 500)
    rd = edge_reads(g, n_random=600, seed=17)
    syn = snapgpu.Reads.synthetic(g, 1500, seed=3, random_read_fraction=0.02)
    rd += [tuple(x.decode() for x in syn.get(i)) for i in range(syn.n)]
    fq = os.path.join(HERE, "small_reads.fq")
    write_fastq(fq, rd)
    idxdir = os.path.join(work, "small_idx")
    ref_index(fa, idxdir)
    for name, params in PARAM_SETS.items():
        with open(os.path.join(HERE, f"expected_small_{name}.tsv"), "w") as f:
            f.write(ref_align(idxdir, fq, params))

    multihit_fixtures(work)
    cigar_fixtures(work)
    refindex_fixtures(work)
    single_fixtures(work)
    paired_fixtures(work)

    # 2. lookupSeed golden: seeds from the genome, their RCs, mutated and random seeds
    rng = random.Random(9)
    seeds = []
    nb = g.n_bases
    while len(seeds) < 3000:
        p = rng.randrange(0, nb - 20)
        s = g.bases(p, 20).decode().upper()
        if set(s) <= set("ACGT"):
            seeds.append(s)
            seeds.append(s.translate(str.maketrans("ACGT", "TGCA"))[::-1])
    seeds += ["".join(rng.choice("ACGT") for _ in range(20)) for _ in range(1000)]
    seeds += ["A" * 20, "T" * 20, "ACGT" * 5, "AATT" * 5, "GATC" * 5]
    with open(os.path.join(HERE, "lookup_seeds.txt"), "w") as f:
        f.write("\n".join(seeds) + "\n")
    with open(os.path.join(HERE, "expected_lookups.tsv"), "w") as f:
        f.write(run([HARNESS, "lookup", idxdir, os.path.join(HERE, "lookup_seeds.txt")]))

    # 3. LV golden vectors (both text directions)
    for direction in (1, -1):
        rows = []
        for _ in range(800):
            L = rng.choice([3, 5, 12, 30, 60, 80, 100, 130])
            t = "".join(rng.choice("ACGT") for _ in range(L + 35))
            p = list(t[:L] if direction > 0 else t[::-1][:L])   # reverse LV walks the text backwards
            for _ in range(rng.randrange(0, 10)):
                op, i = rng.random(), rng.randrange(len(p))
                if op < 0.6:
                    p[i] = rng.choice("ACGTN")
                elif op < 0.8:
                    p.insert(i, rng.choice("ACGT"))
                elif len(p) > 1:
                    del p[i]
            p = "".join(p)
            q = "".join(chr(33 + rng.randrange(0, 45)) for _ in p)
            k = rng.choice([0, 1, 2, 3, 5, 8, 14, 16, 22, 30])
            tl = rng.choice([len(t), len(p) + 31])
            tt = t[:tl] if direction > 0 else t[-tl:]
            rows.append((direction, k, tt, p, q))
        inp = os.path.join(work, f"lv{direction}.tsv")
        with open(inp, "w") as f:
            for r in rows:
                f.write("\t".join(map(str, r)) + "\n")
        out = run([HARNESS, "lv", inp]).splitlines()
        with open(os.path.join(HERE, f"lv_{'fwd' if direction > 0 else 'rev'}.tsv"), "w") as f:
            for r, o in zip(rows, out):
                e, net, prob = o.split("\t")
                f.write("\t".join(map(str, r)) + f"\t{e}\t{net}\t{float.fromhex(prob).hex()}\n")

    # 4. the reference's own datatest fixture (tests/datatest/datatest.{fa,fq})
    for fn in ("datatest.fa", "datatest.fq"):
        shutil.copy(os.path.join("/root/reference/tests/datatest", fn), os.path.join(HERE, fn))
    dt_idx = os.path.join(work, "dt_idx")
    ref_index(os.path.join(HERE, "datatest.fa"), dt_idx)
    with open(os.path.join(HERE, "expected_datatest.tsv"), "w") as f:
        f.write(ref_align(dt_idx, os.path.join(HERE, "datatest.fq"), PARAM_SETS["default"]))

    # 5. digests of the C1 / C2 synthetic configs (inputs regenerated on any host)
    digests = {}
    for cfg in (C1, C2):
        gg = snapgpu.Genome.synthetic(**cfg["genome"])
        gfa = os.path.join(work, f"{cfg['name']}.fa")
        gg.write_fasta(gfa)
        reads = snapgpu.Reads.synthetic(gg, **cfg["reads"])
        rfq = os.path.join(work, f"{cfg['name']}.fq")
        reads.write_fastq(rfq)
        d = os.path.join(work, f"{cfg['name']}_idx")
        ref_index(gfa, d)
        tsv = ref_align(d, rfq, PARAM_SETS["default"])
        digests[cfg["name"]] = {"sha256": digest(tsv), "n": reads.n}
        with open(os.path.join(HERE, f"expected_{cfg['name']}_head.tsv"), "w") as f:
            f.write("".join(tsv.splitlines(True)[:2000]))
    meta["digests"] = digests
    with open(os.path.join(HERE, "golden.json"), "w") as f:
        json.dump(meta, f, indent=1)
    shutil.rmtree(work, ignore_errors=True)
    print("golden fixtures written to", HERE)


if __name__ == "__main__":
    main()
