"""Fixture of tests/test_dupmark_model.py: the reference's own duplicate marks (BAMDupMarkFilter, composed in
front of the compressor by BAMFormat::getWriterSupplier whenever the output is sorted).

Runs where the reference is built (oracle/_ref, the recipe of oracle/Makefile.ref); the tests only read what
it writes:

  dupmark_reads.fq                  the first 300 reads of single_reads.fq, each in 1-5 copies with ids and
                                    qualities (Phred 28-40) of their own; the read at the highest mapped
                                    position in one copy, since the reference never analyses its last run
  expected_dupmark.bam.records.gz   the records of `snap-rna single <genome> <transcriptome> small.gtf
                                    dupmark_reads.fq -t 1 -so -o out.bam`, inflated, header stripped

    python3 tests/golden/make_dupmark_golden.py
"""
import gzip
import os
import random
import shutil
import struct
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SNAP = os.path.join(ROOT, "oracle", "_ref", "snap-rna")


def run(cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def records_of(bam_path):
    """The record stream of a BAM file and the names of its references."""
    raw = gzip.decompress(open(bam_path, "rb").read())
    assert raw[:4] == b"BAM\1"
    at = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    return raw[at:], n_ref


def split(raw):
    at = 0
    while at < len(raw):
        size = 4 + struct.unpack_from("<i", raw, at)[0]
        yield raw[at:at + size]
        at += size


def mapped(r):
    ref, pos = struct.unpack_from("<ii", r, 4)
    return ref >= 0 and pos >= 0 and not struct.unpack_from("<H", r, 18)[0] & 4


def name_of(r):
    return r[36:36 + r[12] - 1].decode()


def main():
    fa, gtf = os.path.join(HERE, "small.fa"), os.path.join(HERE, "small.gtf")
    lines = open(os.path.join(HERE, "single_reads.fq")).read().split("\n")
    reads = [(lines[4 * k][1:].split()[0], lines[4 * k + 1]) for k in range(300)]
    work = tempfile.mkdtemp(prefix="dupmark_golden_")
    try:
        gidx = os.path.join(work, "gidx")
        run([SNAP, "index", fa, gidx])
        run([SNAP, "transcriptome", gtf, fa, "tidx", "-O1000"], cwd=work)

        def align(fq_text, out):
            fq = os.path.join(work, "reads.fq")
            with open(fq, "w") as f:
                f.write(fq_text)
            run([SNAP, "single", gidx, os.path.join(work, "tidx"), gtf, fq, "-t", "1", "-so", "-o", out], cwd=work)
            return records_of(out)

        rng = random.Random(2020)
        quals = lambda n: "".join(chr(33 + rng.randrange(28, 41)) for _ in range(n))
        # one copy of each, to learn which read lies at the highest mapped position
        probe, _ = align("".join(f"@{name}\n{bases}\n+\n{quals(len(bases))}\n" for name, bases in reads),
                         os.path.join(work, "probe.bam"))
        last = [r for r in split(probe) if mapped(r)][-1]
        single = name_of(last)
        text = []
        for name, bases in reads:
            for c in range(1 if name == single else rng.randrange(1, 6)):
                text.append(f"@{name}_copy{c}\n{bases}\n+\n{quals(len(bases))}\n")
        text = "".join(text)
        raw, n_ref = align(text, os.path.join(work, "out.bam"))
        recs = list(split(raw))
        top = [r for r in recs if mapped(r)]
        assert struct.unpack_from("<ii", top[-1], 4) != struct.unpack_from("<ii", top[-2], 4), \
            "the highest mapped position holds more than one read"
        marked = sum(bool(struct.unpack_from("<H", r, 18)[0] & 0x400) for r in recs)
        print(f"{len(recs)} records, {len(top)} mapped, {marked} marked, {n_ref} references")
        with open(os.path.join(HERE, "dupmark_reads.fq"), "w") as f:
            f.write(text)
        with open(os.path.join(HERE, "expected_dupmark.bam.records.gz"), "wb") as f:
            f.write(gzip.compress(raw, compresslevel=9, mtime=0))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
