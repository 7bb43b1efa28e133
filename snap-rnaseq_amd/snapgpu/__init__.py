"""snapgpu -- MI355X-native drop-in for SNAP's BaseAligner hot path.

Python mirror of the reference's C++ surface (SNAPLib/Aligner.h:54-80,
SNAPLib/BaseAligner.h:44-142, SNAPLib/GenomeIndex.h) over the C ABI of
include/snapgpu.h.  Every call goes to the native library: genome/index work is
host C++, alignment is HIP on gfx950.  There is no CPU fallback -- creating a
BaseAligner without a GPU raises.
"""
import ctypes as C
import os
import time

import numpy as np

from . import _ffi
from ._ffi import lib, last_error

NotFound, SingleHit, MultipleHits, UnknownAlignment = 0, 1, 2, 3   # Read.h:41
FORWARD, RC = 0, 1                                                  # directions.h:26-35
InvalidGenomeLocation = 0xFFFFFFFF                                  # Genome.h:29
UnusedScoreValue = 0xFFFF                                           # BaseAligner.h:261

FLAG_READ_TOO_LONG = 0x01
FLAG_MAPQ_FIXED = 0x02
FLAG_DEFERRED = 0x04
FLAG_BYTE_PATH = 0x10
FLAG_TOO_MANY_NS = 0x08
FLAG_NUL_BYTE = 0x20     # a 0x00 byte inside the read: a corrupted upload (no reader produces one)

RESULT_DTYPE = np.dtype([
    ("location", "<u4"), ("score", "<i4"), ("mapq", "<i4"), ("result", "u1"), ("direction", "u1"),
    ("flags", "u1"), ("reserved", "u1"), ("nLookups", "<u4"), ("nLocationsScored", "<u4"),
    ("popularSeedsSkipped", "<u2"), ("nHitsIgnored", "<u2"), ("nProbes", "<u4"), ("nHitWords", "<u4"),
    ("nOverflowLists", "<u4"), ("nElements", "<u4"), ("reserved2", "<u4"),
    ("probabilityOfAllCandidates", "<f8"), ("probabilityOfBestCandidate", "<f8"),
])
assert RESULT_DTYPE.itemsize == C.sizeof(_ffi.Result)

# snapgpu_pair_result_t (include/snapgpu.h): PairedAlignmentResult (PairedEndAligner.h:31-55)
PAIR_RESULT_DTYPE = np.dtype([
    ("location", "<u4", (2,)), ("score", "<i4", (2,)), ("mapq", "<i4", (2,)), ("status", "u1", (2,)),
    ("direction", "u1", (2,)), ("fromAlignTogether", "u1"), ("alignedAsPair", "u1"), ("flags", "<u2"),
    ("nLocationsScored", "<u4"), ("nSingleScored", "<u4"), ("popularSeedsSkipped", "<u4"), ("writtenBy", "<u4"),
    ("probabilityOfAllPairs", "<f8"), ("probabilityOfBestPair", "<f8"),
])
assert PAIR_RESULT_DTYPE.itemsize == 64
PFLAG_POOL_EXHAUSTED, PFLAG_READ_TOO_LONG, PFLAG_DEFERRED, PFLAG_MAPQ_FIXED = 0x01, 0x02, 0x04, 0x08
PFLAG_NUL_BYTE = 0x10

# snapgpu_search_t / snapgpu_multi_hit_t (include/snapgpu.h)
SEARCH_DTYPE = np.dtype([("searchRadius", "<u4"), ("searchLocation", "<u4"), ("searchDirection", "<u4"),
                         ("reserved", "<u4")])
MULTI_HIT_DTYPE = np.dtype([("location", "<u4"), ("direction", "u1"), ("score", "u1"), ("reserved", "<u2")])
MAX_MULTI_HITS_TO_GET = 512   # BaseAligner.h:149


def search_array(search, n):
    """None, a SEARCH_DTYPE array, or an (n, 3) array-like of (radius, location, direction)."""
    if search is None:
        return None
    s = np.asarray(search)
    if s.dtype != SEARCH_DTYPE:
        a = np.asarray(search, dtype=np.uint64).reshape(-1, 3)
        s = np.zeros(len(a), dtype=SEARCH_DTYPE)
        s["searchRadius"], s["searchLocation"], s["searchDirection"] = a[:, 0], a[:, 1], a[:, 2]
    if len(s) != n:
        raise ValueError(f"search has {len(s)} entries for {n} reads")
    return np.ascontiguousarray(s)


class SnapGpuError(RuntimeError):
    pass


_PTR_CALLS = ("genome_from_fasta", "genome_synthetic", "index_build", "index_load", "index_attach", "gtf_load",
              "reads_synthetic",
              "reads_from_fastq", "reads_from_fastq_buffer", "reads_from_arrays", "aligner_create", "reads_upload", "paired_aligner_create",
              "contaminants_create")


def _check(value, what):
    """Pointer-returning calls fail on NULL; int-returning calls on a non-zero code."""
    if what in _PTR_CALLS:
        if not value:
            raise SnapGpuError(f"{what} failed: {last_error()}")
        return value
    if value != 0:
        raise SnapGpuError(f"{what} failed ({value}): {last_error()}")
    return value


def device_cu_count(device=0):
    return lib().snapgpu_device_cu_count(device)


def device_count():
    return lib().snapgpu_device_count()


def host_threads():
    """This rank's host thread budget (snapgpu_host_threads): affinity mask capped by the cgroup
    CPU quota, divided by LOCAL_WORLD_SIZE; SNAPGPU_HOST_THREADS overrides."""
    return lib().snapgpu_host_threads()


class Genome:
    """Whole-genome byte string with contig padding (SNAPLib/Genome.h)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_fasta(cls, path, chromosome_padding=500):
        return cls(_check(lib().snapgpu_genome_from_fasta(str(path).encode(), chromosome_padding), "genome_from_fasta"))

    @classmethod
    def synthetic(cls, total_bases, seed=2121, n_contigs=1, n_repeat_families=200, repeat_fraction=0.45,
                  max_divergence=0.15, n_run_fraction=0.002, chromosome_padding=500):
        p = _ffi.SynthGenomeParams(seed=seed, totalBases=total_bases, nContigs=n_contigs,
                                   nRepeatFamilies=n_repeat_families, repeatFraction=repeat_fraction,
                                   maxDivergence=max_divergence, nRunFraction=n_run_fraction,
                                   chromosomePadding=chromosome_padding)
        return cls(_check(lib().snapgpu_genome_synthetic(C.byref(p)), "genome_synthetic"))

    def write_fasta(self, path):
        _check(lib().snapgpu_genome_write_fasta(self._h, str(path).encode()), "write_fasta")

    @property
    def n_bases(self):
        return lib().snapgpu_genome_nbases(self._h)

    def bases(self, start=0, length=None):
        n = self.n_bases
        if length is None:
            length = n - start
        return C.string_at(lib().snapgpu_genome_bases(self._h) + start, length)

    @property
    def pieces(self):
        L = lib()
        return [(L.snapgpu_genome_piece_name(self._h, i).decode(), L.snapgpu_genome_piece_offset(self._h, i))
                for i in range(L.snapgpu_genome_npieces(self._h))]

    def __del__(self):
        if getattr(self, "_h", None):
            lib().snapgpu_genome_free(self._h)
            self._h = None


class GenomeIndex:
    """Seed index with GenomeIndex::lookupSeed semantics (SNAPLib/GenomeIndex.cpp:971-1086)."""

    def __init__(self, handle, genome_keepalive=None):
        self._h = handle

    @classmethod
    def build(cls, genome, seed_len=20, n_threads=0, slack=0.3, device=None):
        """GenomeIndex::BuildIndexToDirectory semantics with the reference's table sizing
        (slack as `snap-rna index -h`); takes ownership of the genome.  device=None: the CPU
        builder on n_threads host threads.  device=<int>: the same index, byte for byte, built on
        that HIP device (snapgpu_index_build_gpu; n_threads unused); a failure raises, there is no
        fallback to the CPU."""
        h = genome._h
        genome._h = None          # ownership moves to the index
        if device is not None:
            return cls(_check(lib().snapgpu_index_build_gpu(h, seed_len, float(slack), int(device)), "index_build"))
        return cls(_check(lib().snapgpu_index_build_ex(h, seed_len, n_threads, float(slack)), "index_build"))

    @staticmethod
    def gpu_build_stats():
        """Wall seconds by phase and peak device bytes of this process's last build(device=<int>)."""
        t = (C.c_double * len(_ffi.INDEX_BUILD_PHASES))()
        peak = C.c_uint64()
        _check(lib().snapgpu_index_build_gpu_stats(t, C.byref(peak)), "index_build_gpu_stats")
        return {"phase_s": dict(zip(_ffi.INDEX_BUILD_PHASES, list(t))), "peak_device_bytes": peak.value}

    @classmethod
    def load(cls, directory):
        return cls(_check(lib().snapgpu_index_load(str(directory).encode()), "index_load"))

    def share(self, path):
        """Write the flat shared form (one file, e.g. under /dev/shm) for snapgpu_index_attach."""
        _check(lib().snapgpu_index_share(self._h, str(path).encode()), "index_share")

    @classmethod
    def attach(cls, path):
        """Map a shared index read-only (no private copy of the tables)."""
        return cls(_check(lib().snapgpu_index_attach(str(path).encode()), "index_attach"))

    def genome_handle(self):
        """The owned genome (a raw handle for Reads.synthetic; valid while the index lives)."""
        return lib().snapgpu_index_genome(self._h)

    def save(self, directory):
        _check(lib().snapgpu_index_save(self._h, str(directory).encode()), "index_save")

    def info(self):
        i = _ffi.IndexInfo()
        _check(lib().snapgpu_index_get_info(self._h, C.byref(i)), "index_info")
        return {f: getattr(i, f) for f, _ in i._fields_}

    def view(self):
        v = _ffi.IndexView()
        _check(lib().snapgpu_index_get_view(self._h, C.byref(v)), "index_view")
        return v

    def getSeedLength(self):
        return self.info()["seedLen"]

    def genome_bases(self, start, length):
        v = self.view()
        return C.string_at(v.genome + start, length)

    def lookupSeed(self, seed, cap=1 << 20):
        """-> (hits, rcHits): lists of genome offsets (overflow lists descending)."""
        n = (C.c_uint32 * 2)()
        buf = max(1, cap)
        f = (C.c_uint32 * buf)()
        r = (C.c_uint32 * buf)()
        rc = lib().snapgpu_index_lookup(self._h, seed.encode() if isinstance(seed, str) else seed, n, f, r, buf)
        if rc != 0:
            raise SnapGpuError(f"lookup failed: {last_error()}")
        return list(f[:min(n[0], buf)]), list(r[:min(n[1], buf)]), (n[0], n[1])

    def __del__(self):
        if getattr(self, "_h", None):
            lib().snapgpu_index_free(self._h)
            self._h = None


class Reads:
    """A host batch of reads (bases + Phred+33 qualities), Read.h:289-328 contract."""

    def __init__(self, ptr):
        self._p = ptr

    @classmethod
    def synthetic(cls, genome, n_reads, seed=99, read_length=100, quality_char="2", base_error_rate=0.02,
                  mutation_rate=0.001, indel_fraction=0.15, indel_extend=0.3, random_read_fraction=0.0):
        p = _ffi.SynthReadsParams(seed=seed, nReads=n_reads, readLength=read_length,
                                  qualityChar=ord(quality_char), baseErrorRate=base_error_rate,
                                  mutationRate=mutation_rate, indelFraction=indel_fraction,
                                  indelExtend=indel_extend, randomReadFraction=random_read_fraction)
        g = genome._h if isinstance(genome, Genome) else genome
        return cls(_check(lib().snapgpu_reads_synthetic(g, C.byref(p)), "reads_synthetic"))

    @classmethod
    def synthetic_pairs(cls, genome, n_pairs, seed=99, read_length=101, insert_mean=500, insert_sd=50,
                        quality_char="2", base_error_rate=0.02, mutation_rate=0.001, indel_fraction=0.15,
                        indel_extend=0.3):
        """wgsim-like pairs (snapgpu_reads_synthetic_pairs) -> (reads0, reads1)."""
        p = _ffi.SynthReadsParams(seed=seed, nReads=n_pairs, readLength=read_length,
                                  qualityChar=ord(quality_char), baseErrorRate=base_error_rate,
                                  mutationRate=mutation_rate, indelFraction=indel_fraction,
                                  indelExtend=indel_extend, randomReadFraction=0.0)
        g = genome._h if isinstance(genome, Genome) else genome
        a, b = C.POINTER(_ffi.Reads)(), C.POINTER(_ffi.Reads)()
        _check(lib().snapgpu_reads_synthetic_pairs(g, C.byref(p), insert_mean, insert_sd, C.byref(a), C.byref(b)),
               "reads_synthetic_pairs")
        return cls(a), cls(b)

    @classmethod
    def from_fastq(cls, path):
        return cls(_check(lib().snapgpu_reads_from_fastq(str(path).encode()), "reads_from_fastq"))

    @classmethod
    def from_fastq_bytes(cls, data, name="<memory>"):
        """snapgpu_reads_from_fastq_buffer: the host parser over FASTQ text in memory (name only
        appears in error messages)."""
        buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)   # at least one byte to point at
        return cls(_check(lib().snapgpu_reads_from_fastq_buffer(buf.ctypes.data, len(buf) - 1, str(name).encode()),
                          "reads_from_fastq_buffer"))

    @classmethod
    def from_list(cls, reads):
        """reads: iterable of (bases, quals) str/bytes pairs."""
        bases, quals, offs, lens = bytearray(), bytearray(), [], []
        for b, q in reads:
            b = b.encode() if isinstance(b, str) else bytes(b)
            q = q.encode() if isinstance(q, str) else bytes(q)
            if len(q) < len(b):
                q = q + b"!" * (len(b) - len(q))
            offs.append(len(bases))
            lens.append(len(b))
            bases += b
            quals += q[:len(b)]
        n = len(lens)
        bases += b"\0" * 16
        quals += b"\0" * 16
        o = (C.c_uint64 * max(1, n))(*offs)
        l = (C.c_uint32 * max(1, n))(*lens)
        return cls(_check(lib().snapgpu_reads_from_arrays(n, bytes(bases), bytes(quals), o, l), "reads_from_arrays"))

    @classmethod
    def from_arrays(cls, bases, quals, offsets, lengths):
        """snapgpu_reads_from_arrays: read i = bases / quals [offsets[i], + lengths[i]) of two byte
        buffers, taken as they are (any byte value, 0x00 included)."""
        b = np.frombuffer(bytes(bases) + b"\0" * 16, dtype=np.uint8)
        q = np.frombuffer(bytes(quals) + b"\0" * 16, dtype=np.uint8)
        o = np.ascontiguousarray(np.resize(np.asarray(offsets, dtype=np.uint64), max(1, len(lengths))))
        l = np.ascontiguousarray(np.resize(np.asarray(lengths, dtype=np.uint32), max(1, len(lengths))))
        fn = lib().snapgpu_reads_from_arrays
        return cls(_check(fn(len(lengths), C.cast(b.ctypes.data, C.c_char_p), C.cast(q.ctypes.data, C.c_char_p),
                             C.cast(o.ctypes.data, C.POINTER(C.c_uint64)), C.cast(l.ctypes.data, C.POINTER(C.c_uint32))),
                          "reads_from_arrays"))

    def slice(self, start, count):
        """A copy of reads [start, start + count) as a new batch."""
        r = self._p.contents
        count = max(0, min(count, r.n - start))
        offs = C.cast(C.addressof(r.offsets.contents) + 8 * start, C.POINTER(C.c_uint64))
        lens = C.cast(C.addressof(r.lengths.contents) + 4 * start, C.POINTER(C.c_uint32))
        return Reads(_check(lib().snapgpu_reads_from_arrays(count, C.cast(r.bases, C.c_char_p),
                                                            C.cast(r.quals, C.c_char_p), offs, lens),
                            "reads_from_arrays"))

    @property
    def n(self):
        return self._p.contents.n

    def __len__(self):
        return self.n

    def lengths(self):
        """Read lengths as a uint32 array (a copy)."""
        r = self._p.contents
        return np.ctypeslib.as_array(r.lengths, shape=(r.n,)).copy() if r.n else np.zeros(0, np.uint32)

    def get(self, i):
        r = self._p.contents
        o, l = r.offsets[i], r.lengths[i]
        return C.string_at(r.bases + o, l), C.string_at(r.quals + o, l)

    def ids(self):
        """Read ids (FASTQ header without '@'), or None when the batch has none."""
        r = self._p.contents
        if not r.ids:
            return None
        return [C.string_at(r.ids + r.idOffsets[i], r.idLengths[i]) for i in range(r.n)]

    def truth(self):
        r = self._p.contents
        if not r.truthLocation:
            return None
        n = r.n
        loc = np.ctypeslib.as_array(r.truthLocation, shape=(n,)).copy()
        d = np.ctypeslib.as_array(r.truthDirection, shape=(n,)).copy()
        return loc, d

    def clip(self, clipping=3):
        """Read::clip (Read.h:357-404) on every read, in place (the FASTQ reader's step,
        FASTQ.cpp:250; 0 none, 1 front, 2 back, 3 front and back = the reference default).
        -> (frontClipped, unclippedLength) uint32 arrays for sam_format(clip=...)."""
        n = self.n
        front = np.zeros(max(1, n), dtype=np.uint32)
        full = np.zeros(max(1, n), dtype=np.uint32)
        _check(lib().snapgpu_reads_clip(self._p, int(clipping), front.ctypes.data, full.ctypes.data), "reads_clip")
        return front[:n], full[:n]

    def write_fastq(self, path):
        _check(lib().snapgpu_reads_write_fastq(self._p, str(path).encode()), "write_fastq")

    def __del__(self):
        if getattr(self, "_p", None):
            lib().snapgpu_reads_free(self._p)
            self._p = None


def default_params():
    p = _ffi.AlignerParams()
    lib().snapgpu_aligner_params_default(C.byref(p))
    return p


class BaseAligner:
    """GPU BaseAligner (SNAPLib/BaseAligner.h:41-142).

    Constructor arguments follow BaseAligner::BaseAligner (BaseAligner.h:44-55);
    AlignRead follows BaseAligner::AlignRead (BaseAligner.cpp:196-200); AlignReads
    is the batched form the GPU is built for.
    """

    def __init__(self, index, maxHitsToConsider=300, maxK=14, maxReadSize=500, maxSeedsToUse=25,
                 maxSeedCoverage=0.0, extraSearchDepth=2, explorePopularSeeds=False, stopOnFirstHit=False,
                 device=0):
        self.index = index
        self.params = _ffi.AlignerParams(maxHitsToConsider=maxHitsToConsider, maxK=maxK, maxReadSize=maxReadSize,
                                         maxSeedsToUse=maxSeedsToUse, maxSeedCoverage=maxSeedCoverage,
                                         extraSearchDepth=extraSearchDepth,
                                         explorePopularSeeds=int(explorePopularSeeds),
                                         stopOnFirstHit=int(stopOnFirstHit))
        self._h = _check(lib().snapgpu_aligner_create(device, index._h, C.byref(self.params)), "aligner_create")

    def AlignReads(self, reads, out=None):
        """Batched AlignRead -> numpy structured array of RESULT_DTYPE (written into `out`
        when given: a caller streaming batches reuses one record buffer)."""
        n = reads.n
        if out is None:
            out = np.zeros(max(1, n), dtype=RESULT_DTYPE)
        elif out.dtype != RESULT_DTYPE or len(out) < n or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous RESULT_DTYPE array of at least reads.n records")
        if n:
            _check(lib().snapgpu_align_batch(self._h, reads._p, out.ctypes.data_as(C.POINTER(_ffi.Result))),
                   "align_batch")
        return out[:n]

    def submit(self, reads, out):
        """Queue a batch (snapgpu_align_batch_submit); `reads` and `out` stay owned by the caller
        and must not change until wait()."""
        if out.dtype != RESULT_DTYPE or len(out) < reads.n or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous RESULT_DTYPE array of at least reads.n records")
        if reads.n:
            _check(lib().snapgpu_align_batch_submit(self._h, reads._p, out.ctypes.data_as(C.POINTER(_ffi.Result))),
                   "align_batch_submit")

    def wait(self):
        """Finish every submitted batch (snapgpu_align_batch_wait)."""
        _check(lib().snapgpu_align_batch_wait(self._h), "align_batch_wait")

    def AlignReadsEx(self, reads, search=None, maxHitsToGet=0):
        """Batched form of the richer AlignRead (BaseAligner.h:73-86): per-read search
        windows (see search_array) and up to maxHitsToGet multi-hits per read.
        -> (results, multiHitsFound int32[n], multiHits MULTI_HIT_DTYPE[n, maxHitsToGet])."""
        n = reads.n
        out = np.zeros(max(1, n), dtype=RESULT_DTYPE)
        found = np.zeros(max(1, n), dtype=np.int32)
        hits = np.zeros((max(1, n), max(1, maxHitsToGet)), dtype=MULTI_HIT_DTYPE)
        srch = search_array(search, n)
        if n:
            _check(lib().snapgpu_align_batch_ex(self._h, reads._p, None if srch is None else srch.ctypes.data,
                                                maxHitsToGet, out.ctypes.data, found.ctypes.data,
                                                hits.ctypes.data), "align_batch_ex")
        return out[:n], found[:n], hits[:n, :maxHitsToGet]

    def AlignRead(self, bases, quals=None):
        """-> (AlignmentResult, genomeLocation, direction, score, mapq) for one read."""
        if quals is None:
            quals = "I" * len(bases)
        r = self.AlignReads(Reads.from_list([(bases, quals)]))[0]
        return int(r["result"]), int(r["location"]), int(r["direction"]), int(r["score"]), int(r["mapq"])

    def Cigars(self, reads, locations, directions, useM=False):
        """CIGARs as SAMFormat::computeCigarString computes them (SAM.cpp:1162-1230), on
        the GPU, for explicit (location, direction) per read (see cigar_inputs for the
        SAM writer's rules).  -> Cigars(editDistance int32[n], nOps uint32[n],
        ops uint32[n, 64] BAM ops)."""
        n = reads.n
        loc = np.ascontiguousarray(locations, dtype=np.uint32)
        dr = np.ascontiguousarray(directions, dtype=np.uint8)
        assert loc.shape == (n,) and dr.shape == (n,)
        c = Cigars.empty(n)
        if n:
            _check(lib().snapgpu_cigar_batch(self._h, reads._p, loc.ctypes.data, dr.ctypes.data, int(useM),
                                             c.editDistance.ctypes.data, c.nOps.ctypes.data, c.ops.ctypes.data),
                   "cigar_batch")
        return c

    def bucket_info(self):
        """The device bucket image of the seed tables (snapgpu_aligner_bucket_info) as a dict."""
        b = _ffi.BucketInfo()
        _check(lib().snapgpu_aligner_bucket_info(self._h, C.byref(b)), "bucket_info")
        return {f: getattr(b, f) for f, _ in b._fields_}

    def lookup_seeds(self, seeds, mode=0):
        """GenomeIndex::lookupSeed of ACGT seeds on the device, through the bucket image
        (snapgpu_aligner_lookup_seeds; mode 0 = lane per seed, 1 = wave per seed, 2 = four lanes per line).
        -> (uint64[n, 6] {nFwd, nRc, hashFwd, hashRc, firstFwd, firstRc}, uint32[n] lines)."""
        seeds = [s.encode() if isinstance(s, str) else bytes(s) for s in seeds]
        n = len(seeds)
        out = np.zeros((max(1, n), 6), dtype=np.uint64)
        lines = np.zeros(max(1, n), dtype=np.uint32)
        if n:
            _check(lib().snapgpu_aligner_lookup_seeds(self._h, b"".join(seeds), n, int(mode), out.ctypes.data,
                                                       lines.ctypes.data), "lookup_seeds")
        return out[:n], lines[:n]

    def gather_peak_ms(self, n_loads):
        """Diagnostic: best-of-3 time (ms) of n_loads independent random 64-byte bucket-line
        loads from the resident bucket image (roofline calibration for the seed lookups)."""
        ms = C.c_double()
        _check(lib().snapgpu_gather_peak(self._h, int(n_loads), C.byref(ms)), "gather_peak")
        return ms.value

    def set_overlap(self, overlap):
        """Let the pass sets of the two streams run concurrently (default) or one after the other."""
        _check(lib().snapgpu_aligner_set_overlap(self._h, int(bool(overlap))), "set_overlap")

    def set_simple_pass(self, on):
        """Run the single-candidate pass ahead of pass 1 (default) or not; results do not depend on it."""
        _check(lib().snapgpu_aligner_set_simple_pass(self._h, int(bool(on))), "set_simple_pass")

    def debug_trip(self, read_index=0xffffffff):
        """Test hook: trip this aligner's device watchdog when read `read_index` of a batch starts."""
        _check(lib().snapgpu_aligner_debug_trip(self._h, int(read_index)), "debug_trip")

    def debug_grids(self):
        """Test accessor: the persistent kernels' grids and what they were sized from (snapgpu_grids_t)."""
        g = _ffi.Grids()
        _check(lib().snapgpu_aligner_debug_grids(self._h, C.byref(g)), "debug_grids")
        return {f: getattr(g, f) for f, _ in g._fields_}

    def copy_peak_ms(self, nbytes):
        """Diagnostic: best-of-3 time (ms) of a streaming copy of nbytes (read nbytes + write nbytes)."""
        ms = C.c_double()
        _check(lib().snapgpu_copy_peak(self._h, int(nbytes), C.byref(ms)), "copy_peak")
        return ms.value

    def cigar_ms(self):
        ms = C.c_double()
        _check(lib().snapgpu_cigar_last_ms(self._h, C.byref(ms)), "cigar_last_ms")
        return ms.value

    # resident path (bench): upload once, time only the GPU passes
    def sam_format(self, reads, ids, results, cigars, read_group="FASTQ", clip=None, sorted_output=False,
                   return_order=False):
        """The module-level sam_format on the GPU (snapgpu_sam_format_gpu: uploads records and
        CIGARs, runs the resident path's kernels, downloads the text) -> bytes.  sorted_output: the
        lines in coordinate order (`-so`, snapgpu_sam_format_gpu_sorted); return_order (with it):
        -> (bytes, order uint32[n]), order[j] = the read whose line is the j-th."""
        if return_order and not sorted_output:
            raise ValueError("return_order needs sorted_output")
        args, keep, cap = _sam_inputs(reads, ids, results, cigars, read_group, clip)
        used = C.c_uint64()
        buf = np.empty(max(1, cap), dtype=np.uint8)
        order = np.zeros(max(1, reads.n), dtype=np.uint32)
        fn, tail = lib().snapgpu_sam_format_gpu, []
        if sorted_output:
            fn, tail = lib().snapgpu_sam_format_gpu_sorted, [order.ctypes.data if return_order else None]
        rc = fn(self._h, *args, buf.ctypes.data, cap, C.byref(used), *tail)
        if rc != 0 and used.value > cap:
            buf = np.empty(used.value, dtype=np.uint8)
            rc = fn(self._h, *args, buf.ctypes.data, used.value, C.byref(used), *tail)
        _check(rc, "sam_format_gpu")
        text = buf[:used.value].tobytes()
        return (text, order[:reads.n]) if return_order else text

    def sam_ms(self):
        """(kernel ms, download ms) of the last device SAM call (snapgpu_sam_last_ms)."""
        k, d = C.c_double(), C.c_double()
        _check(lib().snapgpu_sam_last_ms(self._h, C.byref(k), C.byref(d)), "sam_last_ms")
        return k.value, d.value

    def sam_pass_ms(self):
        """(length, scan, write) kernel ms of the last device SAM call (snapgpu_sam_pass_ms)."""
        v = [C.c_double() for _ in range(3)]
        _check(lib().snapgpu_sam_pass_ms(self._h, *[C.byref(x) for x in v]), "sam_pass_ms")
        return tuple(x.value for x in v)

    def sam_sort_ms(self):
        """Kernel ms of the sort step of the last device SAM call (snapgpu_sam_sort_ms): 0 after an
        unsorted call."""
        v = C.c_double()
        _check(lib().snapgpu_sam_sort_ms(self._h, C.byref(v)), "sam_sort_ms")
        return v.value

    def bam_format(self, reads, ids, results, cigars, read_group="FASTQ", clip=None, nm_carry=0, sorted_output=False,
                   order=None):
        """The module-level bam_format on the GPU (snapgpu_bam_format_gpu: uploads records and CIGARs,
        runs the resident path's kernels, downloads the records) -> (bytes, NM carry-out).
        sorted_output: the records in coordinate order (the stable order of bam_sort_keys); order: a
        uint32[n] array that then receives that order (order[j] = the read of the j-th record)."""
        if order is not None and not sorted_output:
            raise ValueError("order needs sorted_output")
        if order is not None and (order.dtype != np.uint32 or order.shape != (reads.n,) or not order.flags.c_contiguous):
            raise ValueError("order must be a contiguous uint32 array with one entry per read")
        args, keep, cap = _sam_inputs(reads, ids, results, cigars, read_group, clip)
        used, carry = C.c_uint64(), C.c_int32()
        buf = np.empty(max(1, cap), dtype=np.uint8)
        tail = [int(sorted_output), order.ctypes.data if order is not None and reads.n else None]
        fn = lib().snapgpu_bam_format_gpu
        rc = fn(self._h, *args, int(nm_carry), C.byref(carry), buf.ctypes.data, cap, C.byref(used), *tail)
        if rc != 0 and used.value > cap:
            buf = np.empty(used.value, dtype=np.uint8)
            rc = fn(self._h, *args, int(nm_carry), C.byref(carry), buf.ctypes.data, used.value, C.byref(used), *tail)
        _check(rc, "bam_format_gpu")
        return buf[:used.value].tobytes(), carry.value

    def bam_ms(self):
        """(kernel ms, download ms) of the last device BAM call (snapgpu_bam_last_ms)."""
        k, d = C.c_double(), C.c_double()
        _check(lib().snapgpu_bam_last_ms(self._h, C.byref(k), C.byref(d)), "bam_last_ms")
        return k.value, d.value

    def bgzf_compress(self, data, eof=True):
        """BGZF blocks of `data` compressed on the GPU (snapgpu_bgzf_compress_gpu: uploads the bytes,
        runs the resident path's kernels, downloads the members), then the EOF block if eof -> bytes.
        Byte-identical to the module-level bgzf_compress_model."""
        return _bgzf_call(lambda *tail: lib().snapgpu_bgzf_compress_gpu(self._h, *tail), data, eof, "bgzf_compress_gpu")

    def bgzf_ms(self):
        """(kernel ms, download ms) of the last device BGZF call (snapgpu_bgzf_last_ms)."""
        k, d = C.c_double(), C.c_double()
        _check(lib().snapgpu_bgzf_last_ms(self._h, C.byref(k), C.byref(d)), "bgzf_last_ms")
        return k.value, d.value

    def bai_build(self, records, n_ref, stream_offset=0):
        """(BGZF members without the EOF block, .bai index) of the coordinate-sorted BAM records `records`,
        both made on the GPU (snapgpu_bai_build_gpu: upload, device BGZF, index, two downloads).  The index
        is byte-identical to the module-level bai_build over those members."""
        src = np.frombuffer(bytes(records), dtype=np.uint8)
        n = int(src.size)
        zcap = n + (n // 0xff00 + 1) * 31 + 28
        icap = int(lib().snapgpu_bai_size_bound(n // 36, int(n_ref), n))
        zbuf, ibuf = np.empty(max(1, zcap), dtype=np.uint8), np.empty(max(1, icap), dtype=np.uint8)
        zused, iused = C.c_uint64(), C.c_uint64()
        _check(lib().snapgpu_bai_build_gpu(self._h, src.ctypes.data if n else None, n, int(n_ref), int(stream_offset),
                                           zbuf.ctypes.data, zcap, C.byref(zused), ibuf.ctypes.data, icap, C.byref(iused)),
               "bai_build_gpu")
        return zbuf[:zused.value].tobytes(), ibuf[:iused.value].tobytes()

    def bai_ms(self):
        """(kernel ms, download ms) of the last device BAI call (snapgpu_bai_last_ms)."""
        k, d = C.c_double(), C.c_double()
        _check(lib().snapgpu_bai_last_ms(self._h, C.byref(k), C.byref(d)), "bai_last_ms")
        return k.value, d.value

    def bam_mark_duplicates(self, records, n_ref):
        """(records with FLAG 0x400 on the duplicates, n_marked, n_groups) of the coordinate-sorted single-end
        BAM records `records`, marked on the GPU (snapgpu_bam_mark_duplicates_gpu: upload, the mark passes,
        download).  Byte-identical to the module-level bam_mark_duplicates."""
        buf = np.frombuffer(bytes(records), dtype=np.uint8).copy()
        marked, groups = C.c_uint64(), C.c_uint64()
        _check(lib().snapgpu_bam_mark_duplicates_gpu(self._h, buf.ctypes.data if buf.size else None, int(buf.size), int(n_ref),
                                                     C.byref(marked), C.byref(groups)), "bam_mark_duplicates_gpu")
        return buf.tobytes(), marked.value, groups.value

    def dupmark_ms(self):
        """(kernel ms, download ms) of the last device duplicate marking (snapgpu_bam_dupmark_last_ms)."""
        k, d = C.c_double(), C.c_double()
        _check(lib().snapgpu_bam_dupmark_last_ms(self._h, C.byref(k), C.byref(d)), "bam_dupmark_last_ms")
        return k.value, d.value

    def bgzf_inflate(self, data):
        """The bytes of the BGZF stream `data`, inflated on the GPU (snapgpu_bgzf_inflate_gpu: uploads the
        stream, one wave per member, downloads the bytes).  Byte-identical to the module-level
        bgzf_inflate and bgzf_inflate_model; refuses what they refuse."""
        return _inflate_call(lambda *tail: lib().snapgpu_bgzf_inflate_gpu(self._h, *tail), data, "bgzf_inflate_gpu")

    def bgzf_inflate_ms(self):
        """(upload ms, kernel ms, download ms) of the last device inflate, upload_fastq(bgzf=True)'s
        included (snapgpu_bgzf_inflate_last_ms)."""
        u, k, d = C.c_double(), C.c_double(), C.c_double()
        _check(lib().snapgpu_bgzf_inflate_last_ms(self._h, C.byref(u), C.byref(k), C.byref(d)), "bgzf_inflate_last_ms")
        return u.value, k.value, d.value

    def bgzf_inflate_waves(self):
        """Waves the inflate kernel launches on this aligner's device (snapgpu_bgzf_inflate_waves)."""
        n = lib().snapgpu_bgzf_inflate_waves(self._h)
        if n <= 0:
            raise SnapGpuError(f"bgzf_inflate_waves failed ({n}): {last_error()}")
        return n

    def upload(self, reads):
        return DeviceReads(self, reads)

    def upload_fastq(self, path_or_bytes, clipping=0, host_batch=True, name="<memory>", bgzf=False):
        """FASTQ parsed on the device (snapgpu_fastq_upload / _file): the text (bytes) or the file
        (a path) is uploaded, and split, clipped and packed in device memory -> DeviceReads, as
        upload() of the host parser's batch clipped at `clipping` would give.  Its .reads is that
        host batch (a Reads), or None with host_batch=False.  bgzf=True: the bytes or the file are a
        BGZF stream of the text (bgzip's .gz), inflated on the device (snapgpu_fastq_upload_bgzf /
        _file)."""
        d, r = C.c_void_p(), C.POINTER(_ffi.Reads)()
        flags = FASTQ_HOST_BATCH if host_batch else 0
        rp = C.byref(r) if host_batch else None
        from_bytes, from_file = ((lib().snapgpu_fastq_upload_bgzf, lib().snapgpu_fastq_upload_bgzf_file) if bgzf else
                                 (lib().snapgpu_fastq_upload, lib().snapgpu_fastq_upload_file))
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
            buf = np.frombuffer(bytes(path_or_bytes) + b"\0", dtype=np.uint8)
            rc = from_bytes(self._h, buf.ctypes.data, len(buf) - 1, str(name).encode(), int(clipping), flags, C.byref(d), rp)
        else:
            rc = from_file(self._h, os.fspath(path_or_bytes).encode(), int(clipping), flags, C.byref(d), rp)
        _check(rc, "fastq_upload_bgzf" if bgzf else "fastq_upload")
        return DeviceReads(self, Reads(r) if host_batch else None, handle=d.value)

    def fastq_last_ms(self):
        """(text upload ms, kernel ms, download ms) of the last upload_fastq (snapgpu_fastq_last_ms)."""
        u, k, d = C.c_double(), C.c_double(), C.c_double()
        _check(lib().snapgpu_fastq_last_ms(self._h, C.byref(u), C.byref(k), C.byref(d)), "fastq_last_ms")
        return u.value, k.value, d.value

    def timing(self):
        t = _ffi.Timing()
        lib().snapgpu_last_timing(self._h, C.byref(t))
        return {f: getattr(t, f) for f, _ in t._fields_}

    PHASES = ("setup", "lookup", "insert", "score", "pop", "n_lv_forced_unknown_lowk", "stage", "lv_fwd", "lv_rev", "apply",
              "writeback", "out", "n_pass", "n_cand", "n_lv_forced_unknown_second", "n_pass16", "n_pass32", "n_pass64", "rows_fwd",
              "rows_rev", "n_score_calls", "n_forced", "n_popped", "n_succ", "passloop", "select", "fetch", "seedloop",
              "n_batch", "rank", "n_elems_forced", "candlist", "succ", "nearby", "prob", "fails", "n_fail_steps",
              "succ_tail", "n_pass_forced", "passloop_forced", "heavy_read_cycles", "n_heavy_reads", "n_cand_forced",
              "read_cycles", "n_filter", "n_lv_forced", "n_lv_forced_known", "n_filter_results")

    def phase_cycles(self, reset=True):
        """Diagnostic per-phase shader-cycle sums (needs SNAPGPU_PHASES=1 at construction)."""
        buf = (C.c_uint64 * 48)()
        _check(lib().snapgpu_phase_cycles(self._h, buf, 48, int(reset)), "phase_cycles")
        return {k: int(buf[i]) for i, k in enumerate(self.PHASES)}

    def stats(self):
        s = _ffi.AlignerStats()
        lib().snapgpu_aligner_get_stats(self._h, C.byref(s))
        return {f: getattr(s, f) for f, _ in s._fields_}

    # getters of SNAPLib/Aligner.h:62-77
    def getNHashTableLookups(self):
        return self.stats()["nHashTableLookups"]

    def getLocationsScored(self):
        return self.stats()["nLocationsScored"]

    def getNHitsIgnoredBecauseOfTooHighPopularity(self):
        return self.stats()["nHitsIgnoredBecauseOfTooHighPopularity"]

    def getNReadsIgnoredBecauseOfTooManyNs(self):
        return self.stats()["nReadsIgnoredBecauseOfTooManyNs"]

    def getNIndelsMerged(self):
        return self.stats()["nIndelsMerged"]

    def getMaxK(self):
        return lib().snapgpu_aligner_max_k(self._h)

    def getName(self):
        return lib().snapgpu_aligner_name(self._h).decode()

    def __del__(self):
        if getattr(self, "_h", None):
            lib().snapgpu_aligner_free(self._h)
            self._h = None


def paired_params(**kw):
    """snapgpu_paired_params_t with the paired CLI defaults, overridden by kw."""
    p = _ffi.PairedParams()
    lib().snapgpu_paired_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class PairedAligner:
    """GPU ChimericPairedEndAligner over an IntersectingPairedEndAligner, constructed as
    PairedAligner.cpp:462-482 does (SNAPLib/ChimericPairedEndAligner.h, IntersectingPairedEndAligner.h).
    align() is ChimericPairedEndAligner::align for every pair; intersect() the intersecting aligner
    alone.  Keyword arguments: snapgpu_paired_params_t fields (maxHits, maxK, maxSeedsToUse,
    extraSearchDepth, minSpacing, maxSpacing, maxBigHits, maxCandidatePoolSize, maxReadSize,
    forceSpacing, seedCoverage)."""

    def __init__(self, index, device=0, **kw):
        self.index = index
        self.params = paired_params(**kw)
        self._h = _check(lib().snapgpu_paired_aligner_create(device, index._h, C.byref(self.params)),
                         "paired_aligner_create")

    def _run(self, fn, reads0, reads1, what):
        if reads0.n != reads1.n:
            raise ValueError("the two read batches differ in length")
        out = np.zeros(max(1, reads0.n), dtype=PAIR_RESULT_DTYPE)
        if reads0.n:
            _check(fn(self._h, reads0._p, reads1._p, out.ctypes.data), what)
        return out[:reads0.n]

    def align(self, reads0, reads1):
        return self._run(lib().snapgpu_paired_align_batch, reads0, reads1, "paired_align_batch")

    def intersect(self, reads0, reads1):
        return self._run(lib().snapgpu_paired_intersect_batch, reads0, reads1, "paired_intersect_batch")

    def debug_grids(self):
        """Test accessor (snapgpu_paired_aligner_debug_grids): the pair kernels' grids and their source."""
        out = (C.c_uint32 * 8)()
        _check(lib().snapgpu_paired_aligner_debug_grids(self._h, out), "paired debug_grids")
        names = ("computeUnits", "perCU128", "grid128", "perCU256", "grid256", "perCU512", "grid512", "gridPools")
        return dict(zip(names, (int(v) for v in out)))

    # the resident pair batch: what the last align() / intersect() left in HBM
    def resident_pairs(self):
        """Pairs of the batch the aligner's last intersecting run left resident (0: none)."""
        return int(lib().snapgpu_paired_resident_pairs(self._h))

    def run_cigars(self, results, useM=False):
        """CIGARs of both ends of the resident batch at the locations and directions of `results`
        (the caller's final records of that batch), over the bases already in HBM (asynchronous)."""
        res = np.ascontiguousarray(results, dtype=PAIR_RESULT_DTYPE)
        n = self.resident_pairs()
        if n and res.shape != (n,):   # the C call takes no count: it reads one record per resident pair
            raise ValueError(f"results has shape {res.shape} for the {n} pairs of the resident batch")
        _check(lib().snapgpu_paired_cigar_resident(self._h, res.ctypes.data if n else None, int(useM)),
               "paired_cigar_resident")

    def cigars(self):
        """The 2n rows run_cigars() wrote (waits): row 2q + e is end e of pair q."""
        c = Cigars.empty(2 * self.resident_pairs())   # the C call writes two rows per resident pair
        _check(lib().snapgpu_paired_cigar_download(self._h, c.editDistance.ctypes.data, c.nOps.ctypes.data,
                                                   c.ops.ctypes.data), "paired_cigar_download")
        return c

    def run_sam(self, reads0, reads1, read_group="FASTQ"):
        """SAM lines of the resident batch, its uploaded records and the CIGARs run_cigars() left in
        HBM, formatted on the GPU (asynchronous).  reads0 / reads1: the batches that were aligned
        (their ids and clip state are uploaded, their bases are not)."""
        rg = None if read_group is None else (read_group.encode() if isinstance(read_group, str) else bytes(read_group))
        _check(lib().snapgpu_paired_sam_resident(self._h, reads0._p, reads1._p, rg), "paired_sam_resident")

    def sam(self, timing=None):
        """The text run_sam() wrote -> bytes (waits).  timing: a dict that receives "done", the
        time.perf_counter() at which the text was in host memory."""
        used = C.c_uint64()
        fn = lib().snapgpu_paired_sam_download
        rc = fn(self._h, None, 0, C.byref(used))
        if rc != 0 and used.value == 0:
            _check(rc, "paired_sam_download")
        buf = np.empty(max(1, used.value), dtype=np.uint8)
        _check(fn(self._h, buf.ctypes.data, used.value, C.byref(used)), "paired_sam_download")
        if timing is not None:
            timing["done"] = time.perf_counter()
        return buf[:used.value].tobytes()

    def sam_format(self, reads0, reads1, results, cigars, read_group="FASTQ"):
        """The module-level sam_format_pairs on the GPU (snapgpu_sam_format_pairs_gpu: uploads reads,
        records and CIGARs, runs the resident path's kernels, downloads the text) -> bytes."""
        args, keep, cap = _pair_inputs(self.index, reads0, reads1, results, cigars, read_group)
        return _sized_call(lambda *a: lib().snapgpu_sam_format_pairs_gpu(self._h, *a), args, cap, "sam_format_pairs_gpu")

    def sam_ms(self):
        """(CIGAR kernel ms, formatter kernel ms, download ms) of the last resident calls
        (snapgpu_paired_sam_last_ms)."""
        v = [C.c_double() for _ in range(3)]
        _check(lib().snapgpu_paired_sam_last_ms(self._h, *[C.byref(x) for x in v]), "paired_sam_last_ms")
        return tuple(x.value for x in v)

    def run_bam(self, reads0, reads1, read_group="FASTQ", sorted_output=False, nm_carry=0):
        """BAM records of the resident batch, its uploaded records and the CIGARs run_cigars() left in
        HBM, encoded on the GPU (asynchronous).  reads0 / reads1: as run_sam(); sorted_output: the
        records in coordinate order, bam_order() then gives that order; nm_carry: the NM that ends
        without location repeat until the first end with one (the previous batch's bam_nm_carry())."""
        rg = None if read_group is None else (read_group.encode() if isinstance(read_group, str) else bytes(read_group))
        fn = lib().snapgpu_paired_bam_resident_sorted if sorted_output else lib().snapgpu_paired_bam_resident
        _check(fn(self._h, reads0._p, reads1._p, rg, int(nm_carry)), "paired_bam_resident")
        self._bam_carry = None

    def bam(self, timing=None):
        """The records run_bam() wrote -> bytes (waits).  timing: as sam()."""
        used, carry = C.c_uint64(), C.c_int32()
        fn = lib().snapgpu_paired_bam_download
        rc = fn(self._h, None, 0, C.byref(used), C.byref(carry))
        if rc != 0 and used.value == 0:
            _check(rc, "paired_bam_download")
        buf = np.empty(max(1, used.value), dtype=np.uint8)
        _check(fn(self._h, buf.ctypes.data, used.value, C.byref(used), C.byref(carry)), "paired_bam_download")
        if timing is not None:
            timing["done"] = time.perf_counter()
        self._bam_carry = carry.value
        return buf[:used.value].tobytes()

    def bam_nm_carry(self):
        """The NM carry-out of the last run_bam() (waits): the nm_carry of the next batch."""
        if getattr(self, "_bam_carry", None) is None:
            used, carry = C.c_uint64(), C.c_int32()
            rc = lib().snapgpu_paired_bam_download(self._h, None, 0, C.byref(used), C.byref(carry))
            if rc != 0 and used.value == 0:
                _check(rc, "paired_bam_download")
            self._bam_carry = carry.value
        return self._bam_carry

    def bam_order(self):
        """The output order of the last run_bam(sorted_output=True) -> uint32[2n] (waits): order[j] is
        the write-order index 2q + w of the j-th record."""
        n = 2 * self.resident_pairs()
        order = np.zeros(max(1, n), dtype=np.uint32)
        _check(lib().snapgpu_paired_bam_order_download(self._h, order.ctypes.data), "paired_bam_order_download")
        return order[:n]

    def bam_format(self, reads0, reads1, results, cigars, read_group="FASTQ", nm_carry=0, sorted_output=False,
                   order=None):
        """The module-level bam_format_pairs on the GPU (snapgpu_bam_format_pairs_gpu: uploads reads,
        records and CIGARs, runs the resident path's kernels, downloads the records) -> (bytes, NM
        carry-out).  sorted_output: the records in coordinate order (the stable order of
        bam_pair_sort_keys); order: a uint32[2n] array that then receives that order."""
        if order is not None and not sorted_output:
            raise ValueError("order needs sorted_output")
        if order is not None and (order.dtype != np.uint32 or order.shape != (2 * reads0.n,) or not order.flags.c_contiguous):
            raise ValueError("order must be a contiguous uint32 array with two entries per pair")
        args, keep, cap = _pair_inputs(self.index, reads0, reads1, results, cigars, read_group)
        tail = [int(sorted_output), order.ctypes.data if order is not None and reads0.n else None]
        return _carry_call(lambda *a: lib().snapgpu_bam_format_pairs_gpu(self._h, *a), args, nm_carry, cap,
                           "bam_format_pairs_gpu", tail)

    def bam_ms(self):
        """(encoder kernel ms, download ms) of the last resident BAM calls (snapgpu_paired_bam_last_ms)."""
        k, d = C.c_double(), C.c_double()
        _check(lib().snapgpu_paired_bam_last_ms(self._h, C.byref(k), C.byref(d)), "paired_bam_last_ms")
        return k.value, d.value

    def __del__(self):
        if getattr(self, "_h", None):
            lib().snapgpu_paired_aligner_free(self._h)
            self._h = None


SEED_RUN_DTYPE = np.dtype([("location", "<u4"), ("minOffset", "<u2"), ("maxOffset", "<u2"), ("count", "<u2"),
                           ("direction", "u1"), ("reserved", "u1")])


def charseeds_params(**kw):
    """snapgpu_charseeds_params_t: the partial aligner of PairedAligner.cpp:518-527 by default."""
    p = _ffi.CharSeedsParams()
    lib().snapgpu_charseeds_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def characterize_seeds(aligner, reads, read_list=None, **kw):
    """BaseAligner::CharacterizeSeeds (BaseAligner.cpp:206-508) on the GPU over `reads` (or the
    reads at indices read_list), on the index of `aligner`.  -> (start uint64[n+1],
    nForward uint32[n], flags uint32[n], runs SEED_RUN_DTYPE[...]): read i's map entries are
    runs[start[i]:start[i+1]], the first nForward[i] of them from `map`, the rest from `mapRC`."""
    p = charseeds_params(**kw)
    lst = None if read_list is None else np.ascontiguousarray(read_list, dtype=np.uint64)
    h = lib().snapgpu_characterize_seeds(aligner._h, reads._p, None if lst is None else lst.ctypes.data,
                                         0 if lst is None else len(lst), C.byref(p))
    if not h:
        raise SnapGpuError(f"characterize_seeds: {last_error()}")
    try:
        r = h.contents
        n = r.n
        start = np.ctypeslib.as_array(r.start, shape=(n + 1,)).copy()
        nfwd = np.ctypeslib.as_array(r.nForward, shape=(max(1, n),))[:n].copy()
        flags = np.ctypeslib.as_array(r.flags, shape=(max(1, n),))[:n].copy()
        runs = np.zeros(r.nRuns, dtype=SEED_RUN_DTYPE)
        if r.nRuns:
            C.memmove(runs.ctypes.data, r.runs, r.nRuns * SEED_RUN_DTYPE.itemsize)
    finally:
        lib().snapgpu_seed_runs_free(h)
    return start, nfwd, flags, runs


class DeviceReads:
    def __init__(self, aligner, reads, handle=None):
        """Uploads `reads`; or, with `handle`, adopts a resident batch that already exists
        (BaseAligner.upload_fastq: reads is then its host batch, or None)."""
        self.aligner = aligner
        self.reads = reads
        if handle is None:
            self.n = reads.n
            self._h = _check(lib().snapgpu_reads_upload(aligner._h, reads._p), "reads_upload")
        else:
            self._h = handle
            self.n = self.peek(arrays=False)["n"]

    def peek(self, arrays=True):
        """The resident batch as the device holds it (snapgpu_device_reads_peek; for the tests) ->
        dict of n, bytes, maxLen, extentHash and, with arrays, offsets, lengths, bases and quals
        (bytes + 64 each)."""
        n, nb, ml, eh = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
        fn = lib().snapgpu_device_reads_peek
        _check(fn(self.aligner._h, self._h, C.byref(n), C.byref(nb), C.byref(ml), C.byref(eh), None, None, None, None),
               "device_reads_peek")
        out = {"n": n.value, "bytes": nb.value, "maxLen": ml.value, "extentHash": eh.value}
        if arrays:
            off, ln = np.zeros(max(1, n.value), np.uint64), np.zeros(max(1, n.value), np.uint32)
            b, q = np.zeros(nb.value + 64, np.uint8), np.zeros(nb.value + 64, np.uint8)
            _check(fn(self.aligner._h, self._h, None, None, None, None, off.ctypes.data, ln.ctypes.data,
                      b.ctypes.data, q.ctypes.data), "device_reads_peek")
            out.update(offsets=off[:n.value], lengths=ln[:n.value], bases=b.tobytes(), quals=q.tobytes())
        return out

    def ids(self):
        """The resident ids and clip state of a batch from upload_fastq
        (snapgpu_device_reads_ids_download; waits) -> (list of bytes, front clips, unclipped lengths):
        what Reads.ids() and Reads.clip() give for the host batch.  The two arrays are None for a
        batch uploaded with clipping 0 (and for an empty one)."""
        fn = lib().snapgpu_device_reads_ids_download
        used = C.c_uint64()
        rc = fn(self.aligner._h, self._h, None, 0, C.byref(used), None, None, None, None)
        if rc != 0 and used.value == 0:
            _check(rc, "device_reads_ids_download")
        n = self.n
        blob = np.zeros(max(1, used.value), np.uint8)
        off, ln = np.zeros(max(1, n), np.uint64), np.zeros(max(1, n), np.uint32)
        untouched = 0xffffffff                       # no length reaches it
        front, full = np.full(max(1, n), untouched, np.uint32), np.full(max(1, n), untouched, np.uint32)
        _check(fn(self.aligner._h, self._h, blob.ctypes.data, used.value, C.byref(used), off.ctypes.data,
                  ln.ctypes.data, front.ctypes.data, full.ctypes.data), "device_reads_ids_download")
        raw = blob.tobytes()
        out = [raw[int(o):int(o) + int(l)] for o, l in zip(off[:n], ln[:n])]
        if n == 0 or full[0] == untouched:
            return out, None, None
        return out, front[:n], full[:n]

    def run(self):
        """Launch the GPU passes (asynchronous)."""
        _check(lib().snapgpu_align_resident(self.aligner._h, self._h), "align_resident")

    def synchronize(self):
        _check(lib().snapgpu_synchronize(self.aligner._h), "synchronize")

    def results(self):
        out = np.zeros(max(1, self.n), dtype=RESULT_DTYPE)
        _check(lib().snapgpu_results_download(self.aligner._h, self._h,
                                              out.ctypes.data_as(C.POINTER(_ffi.Result))), "results_download")
        return out[:self.n]

    def run_cigars(self, useM=False):
        """CIGARs of the records the last run() left in HBM (asynchronous)."""
        _check(lib().snapgpu_cigar_resident(self.aligner._h, self._h, int(useM)), "cigar_resident")

    def cigars(self):
        c = Cigars.empty(self.n)
        _check(lib().snapgpu_cigar_download(self.aligner._h, self._h, c.editDistance.ctypes.data,
                                            c.nOps.ctypes.data, c.ops.ctypes.data), "cigar_download")
        return c

    def run_sam(self, reads=None, ids=None, read_group="FASTQ", sorted_output=False):
        """SAM lines of the records and CIGARs run() + run_cigars() left in HBM, formatted on the
        GPU (asynchronous).  reads: the batch this was uploaded from, or None for the resident ids
        and clip state of a batch from upload_fastq (no host batch needed); ids: None for its own ids;
        sorted_output: the lines in coordinate order (`-so`), sam_order() then gives that order."""
        rg = None if read_group is None else read_group.encode()
        if ids is None:
            self._sam_keep = None
            args = [None, None, None]
        else:
            blob, offs, lens = _id_arrays(ids, self.n if reads is None else reads.n)
            self._sam_keep = (blob, offs, lens)
            args = [blob, offs.ctypes.data, lens.ctypes.data]
        fn = lib().snapgpu_sam_resident_sorted if sorted_output else lib().snapgpu_sam_resident
        _check(fn(self.aligner._h, self._h, None if reads is None else reads._p, *args, rg), "sam_resident")

    def sam_order(self):
        """The output order of the last run_sam(sorted_output=True) -> uint32[n] (waits): entry j is
        the read whose line is the j-th of sam()'s text."""
        order = np.zeros(max(1, self.n), dtype=np.uint32)
        _check(lib().snapgpu_sam_order_download(self.aligner._h, self._h, order.ctypes.data), "sam_order_download")
        return order[:self.n]

    def sam(self, timing=None):
        """The text run_sam() wrote -> bytes (waits).  timing: a dict that receives "done", the
        time.perf_counter() at which the text was in host memory."""
        used = C.c_uint64()
        fn = lib().snapgpu_sam_download
        rc = fn(self.aligner._h, self._h, None, 0, C.byref(used))
        if rc != 0 and used.value == 0:
            _check(rc, "sam_download")
        buf = np.empty(max(1, used.value), dtype=np.uint8)
        _check(fn(self.aligner._h, self._h, buf.ctypes.data, used.value, C.byref(used)), "sam_download")
        if timing is not None:
            timing["done"] = time.perf_counter()
        return buf[:used.value].tobytes()

    def run_bam(self, reads=None, ids=None, read_group="FASTQ", sorted_output=False, nm_carry=0):
        """BAM records of the records and CIGARs run() + run_cigars() left in HBM, encoded on the GPU
        (asynchronous).  reads: the batch this was uploaded from, or None as in run_sam(); ids: None
        for its own ids;
        sorted_output: the records in coordinate order, bam_order() then gives that order; nm_carry:
        the NM that records without CIGAR ops repeat until the first record with ops (the previous
        batch's bam_nm_carry())."""
        rg = None if read_group is None else read_group.encode()
        if ids is None:
            self._bam_keep = None
            args = [None, None, None]
        else:
            blob, offs, lens = _id_arrays(ids, self.n if reads is None else reads.n)
            self._bam_keep = (blob, offs, lens)
            args = [blob, offs.ctypes.data, lens.ctypes.data]
        fn = lib().snapgpu_bam_resident_sorted if sorted_output else lib().snapgpu_bam_resident
        _check(fn(self.aligner._h, self._h, None if reads is None else reads._p, *args, rg, int(nm_carry)),
               "bam_resident")
        self._bam_carry = None

    def bam_order(self):
        """The output order of the last run_bam(sorted_output=True) -> uint32[n] (waits)."""
        order = np.zeros(max(1, self.n), dtype=np.uint32)
        _check(lib().snapgpu_bam_order_download(self.aligner._h, self._h, order.ctypes.data), "bam_order_download")
        return order[:self.n]

    def bam(self, timing=None):
        """The records run_bam() wrote -> bytes (waits).  timing: as sam()."""
        used, carry = C.c_uint64(), C.c_int32()
        fn = lib().snapgpu_bam_download
        rc = fn(self.aligner._h, self._h, None, 0, C.byref(used), C.byref(carry))
        if rc != 0 and used.value == 0:
            _check(rc, "bam_download")
        buf = np.empty(max(1, used.value), dtype=np.uint8)
        _check(fn(self.aligner._h, self._h, buf.ctypes.data, used.value, C.byref(used), C.byref(carry)), "bam_download")
        if timing is not None:
            timing["done"] = time.perf_counter()
        self._bam_carry = carry.value
        return buf[:used.value].tobytes()

    def bam_nm_carry(self):
        """The NM carry-out of the last run_bam() (waits): the nm_carry of the next batch."""
        if getattr(self, "_bam_carry", None) is None:
            used, carry = C.c_uint64(), C.c_int32()
            rc = lib().snapgpu_bam_download(self.aligner._h, self._h, None, 0, C.byref(used), C.byref(carry))
            if rc != 0 and used.value == 0:
                _check(rc, "bam_download")
            self._bam_carry = carry.value
        return self._bam_carry

    def run_bgzf(self):
        """BGZF members of the records the last run_bam() wrote, compressed on the GPU (asynchronous;
        snapgpu_bam_bgzf_resident).  A later run_bam() invalidates them."""
        _check(lib().snapgpu_bam_bgzf_resident(self.aligner._h, self._h), "bam_bgzf_resident")

    def bgzf(self, eof=True, timing=None):
        """The members run_bgzf() wrote, then the EOF block if eof -> bytes (waits).  timing: as sam()."""
        used = C.c_uint64()
        fn = lib().snapgpu_bam_bgzf_download
        rc = fn(self.aligner._h, self._h, int(bool(eof)), None, 0, C.byref(used))
        if rc != 0 and used.value == 0:
            _check(rc, "bam_bgzf_download")
        buf = np.empty(max(1, used.value), dtype=np.uint8)
        _check(fn(self.aligner._h, self._h, int(bool(eof)), buf.ctypes.data, used.value, C.byref(used)), "bam_bgzf_download")
        if timing is not None:
            timing["done"] = time.perf_counter()
        return buf[:used.value].tobytes()

    def run_dupmark(self):
        """Mark the duplicates (FLAG 0x400) among the records of the last run_bam(sorted_output=True), where
        they lie on the GPU (asynchronous; snapgpu_bam_dupmark_resident).  bam() then returns the marked
        records; an earlier run_bgzf() or run_bai() is stale and has to be run again.  A later run_bam()
        writes the records again, unmarked."""
        _check(lib().snapgpu_bam_dupmark_resident(self.aligner._h, self._h), "bam_dupmark_resident")

    def dupmark_stats(self):
        """(n_marked, n_groups) of the last run_dupmark() (waits): the records that carry 0x400 and the
        groups of two or more."""
        marked, groups = C.c_uint64(), C.c_uint64()
        _check(lib().snapgpu_bam_dupmark_stats(self.aligner._h, self._h, C.byref(marked), C.byref(groups)), "bam_dupmark_stats")
        return marked.value, groups.value

    def run_bai(self, stream_offset=0):
        """The .bai index of the records of the last run_bam(sorted_output=True) over the members of the
        run_bgzf() after it, built on the GPU (asynchronous; snapgpu_bam_bai_resident).  stream_offset:
        the compressed bytes ahead of the members in the file (the BGZF of the BAM header).  A later
        run_bam() or run_bgzf() invalidates it."""
        _check(lib().snapgpu_bam_bai_resident(self.aligner._h, self._h, int(stream_offset)), "bam_bai_resident")

    def bai(self, timing=None):
        """The index run_bai() built -> bytes (waits).  timing: as sam()."""
        used = C.c_uint64()
        fn = lib().snapgpu_bam_bai_download
        rc = fn(self.aligner._h, self._h, None, 0, C.byref(used))
        if rc != 0 and used.value == 0:
            _check(rc, "bam_bai_download")
        buf = np.empty(max(1, used.value), dtype=np.uint8)
        _check(fn(self.aligner._h, self._h, buf.ctypes.data, used.value, C.byref(used)), "bam_bai_download")
        if timing is not None:
            timing["done"] = time.perf_counter()
        return buf[:used.value].tobytes()

    def __del__(self):
        if getattr(self, "_h", None):
            lib().snapgpu_device_reads_free(self._h)
            self._h = None


# the device FASTQ parser (include/snapgpu.h; csrc/fastq_parse.h: kTileBytes)
FASTQ_HOST_BATCH = 1
FASTQ_TILE_BYTES = 16384

# the device SAM formatter's work split (csrc/sam_format.h: kRecsPerGroup, kScanTile)
SAM_RECORDS_PER_WORKGROUP = 32
SAM_SCAN_TILE = 2048

CIGAR_OPS = "MIDNSHP=X"   # BAM op codes (SAM spec; BAMAlignment::CigarToCode)


class Cigars:
    """Per-read CIGAR results: editDistance (NM, -1 = "*"), nOps, ops (BAM-encoded)."""

    def __init__(self, editDistance, nOps, ops):
        self.editDistance, self.nOps, self.ops = editDistance, nOps, ops

    @classmethod
    def empty(cls, n):
        return cls(np.full(max(1, n), -1, dtype=np.int32)[:n], np.zeros(max(1, n), dtype=np.uint32)[:n],
                   np.zeros((max(1, n), _ffi.CIGAR_MAX_OPS), dtype=np.uint32)[:n])

    def string(self, i):
        """COMPACT_CIGAR_STRING form (LandauVishkin.cpp:49-62), or "*"."""
        if self.editDistance[i] < 0:
            return "*"
        return "".join(f"{int(o) >> 4}{CIGAR_OPS[int(o) & 15]}" for o in self.ops[i, :self.nOps[i]])


def cigar_inputs(results):
    """(locations, directions) the SAM writer computes CIGARs for (SAM.cpp:1007-1048,
    855-883): writeRead's own location, the forward read unless the read is mapped RC."""
    loc = np.ascontiguousarray(results["location"], dtype=np.uint32)
    mapped = (results["result"] != NotFound) & (loc != 0xFFFFFFFF)
    return loc, np.where(mapped, results["direction"], 0).astype(np.uint8)


def sam_header(index, command_line, version, sorted_output=False, rg_line=None):
    """SAM header (SAMFormat::writeHeader, SAM.cpp:700-800) for a FASTQ input -> bytes."""
    used = C.c_uint64()
    args = [index._h, int(sorted_output), command_line.encode(), version.encode(),
            None if rg_line is None else rg_line.encode()]
    lib().snapgpu_sam_header(*args, None, 0, C.byref(used))
    buf = C.create_string_buffer(max(1, used.value))
    _check(lib().snapgpu_sam_header(*args, buf, used.value, C.byref(used)), "sam_header")
    return C.string_at(buf, used.value)


def sam_format(index, reads, ids, results, cigars, read_group="FASTQ", clip=None, timing=None):
    """SAM lines (SAMFormat::writeRead, SAM.cpp:1007-1155) of single-end genome
    alignments -> bytes.  ids: list of read ids (str/bytes); clip: the (frontClipped,
    unclippedLength) pair Reads.clip returned, or None for unclipped reads; timing: a dict that
    receives the seconds spent in the C formatter ("format_s")."""
    n = reads.n
    idb = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
    assert len(idb) == n
    lens = np.array([len(x) for x in idb], dtype=np.uint32)
    offs = np.zeros(max(1, n), dtype=np.uint64)
    if n > 1:
        offs[1:n] = np.cumsum(lens[:-1], dtype=np.uint64)
    blob = b"".join(idb) + b"\0"
    res = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
    used = C.c_uint64()
    rg = None if read_group is None else read_group.encode()
    args = [index._h, reads._p, blob, offs.ctypes.data, lens.ctypes.data, res.ctypes.data,
            cigars.editDistance.ctypes.data, cigars.nOps.ctypes.data, cigars.ops.ctypes.data, rg]
    fn = lib().snapgpu_sam_format
    if clip is not None:
        front = np.ascontiguousarray(clip[0], dtype=np.uint32)
        full = np.ascontiguousarray(clip[1], dtype=np.uint32)
        assert front.shape == (n,) and full.shape == (n,)
        args += [front.ctypes.data, full.ctypes.data]
        fn = lib().snapgpu_sam_format_clipped
    # one formatting pass with a generous (uninitialised) buffer; a second only if it was too small
    cap = int(lens.sum()) + 2 * int(reads._p.contents.totalBytes) + n * 512
    buf = np.empty(max(1, cap), dtype=np.uint8)
    t0 = time.perf_counter()
    rc = fn(*args, buf.ctypes.data, cap, C.byref(used))
    if rc != 0:
        buf = np.empty(max(1, used.value), dtype=np.uint8)
        t0 = time.perf_counter()
        _check(fn(*args, buf.ctypes.data, used.value, C.byref(used)), "sam_format")
    if timing is not None:
        timing["format_s"] = time.perf_counter() - t0
    return buf[:used.value].tobytes()


def _id_arrays(ids, n):
    """ids (str/bytes) -> (blob, offsets u64, lengths u32) as the C formatters take them."""
    idb = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
    if len(idb) != n:
        raise ValueError(f"{len(idb)} ids for {n} reads")
    lens = np.zeros(max(1, n), dtype=np.uint32)
    lens[:n] = [len(x) for x in idb]
    offs = np.zeros(max(1, n), dtype=np.uint64)
    if n > 1:
        offs[1:n] = np.cumsum(lens[:n - 1], dtype=np.uint64)
    return b"".join(idb) + b"\0", offs, lens


def _sam_inputs(reads, ids, results, cigars, read_group, clip):
    """The argument list snapgpu_sam_format_clipped takes after the index (and what keeps it alive)."""
    n = reads.n
    blob, offs, lens = _id_arrays(ids, n)
    res = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
    if res.shape != (n,) or len(cigars.editDistance) != n:
        raise ValueError("results / cigars do not have one entry per read")
    ed = np.ascontiguousarray(cigars.editDistance, dtype=np.int32)
    nops = np.ascontiguousarray(cigars.nOps, dtype=np.uint32)
    ops = np.ascontiguousarray(cigars.ops, dtype=np.uint32)
    rg = None if read_group is None else (read_group.encode() if isinstance(read_group, str) else bytes(read_group))
    front = full = None
    if clip is not None:
        front = np.ascontiguousarray(clip[0], dtype=np.uint32)
        full = np.ascontiguousarray(clip[1], dtype=np.uint32)
        if front.shape != (n,) or full.shape != (n,):
            raise ValueError("clip arrays do not have one entry per read")
    keep = (blob, offs, lens, res, ed, nops, ops, rg, front, full)
    ptr = lambda a: None if a is None else (a.ctypes.data if a.size else np.zeros(1, a.dtype).ctypes.data)
    if n == 0:   # zero-size arrays have no address worth passing
        keep += tuple(np.zeros(1, dtype=t) for t in (RESULT_DTYPE, np.int32, np.uint32, np.uint32))
        args = [reads._p, blob, offs.ctypes.data, lens.ctypes.data, keep[-4].ctypes.data, keep[-3].ctypes.data,
                keep[-2].ctypes.data, keep[-1].ctypes.data, rg, None, None]
    else:
        args = [reads._p, blob, offs.ctypes.data, lens.ctypes.data, res.ctypes.data, ed.ctypes.data, nops.ctypes.data,
                ops.ctypes.data, rg, ptr(front), ptr(full)]
    return args, keep, int(lens[:n].sum()) + 2 * int(reads._p.contents.totalBytes) + n * 512


def sam_line_lengths(index, reads, ids, results, cigars, read_group="FASTQ", clip=None):
    """Byte length of every line sam_format prints (snapgpu_sam_line_lengths: the host side of the
    device formatter's length pass; needs no GPU) -> np.uint32 array."""
    args, keep, _ = _sam_inputs(reads, ids, results, cigars, read_group, clip)
    out = np.zeros(max(1, reads.n), dtype=np.uint32)
    _check(lib().snapgpu_sam_line_lengths(index._h, *args, out.ctypes.data), "sam_line_lengths")
    return out[:reads.n]


def _pair_inputs(index, reads0, reads1, results, cigars, read_group):
    """The argument list the pair formatters take up to the read group (and what keeps it alive)."""
    n = reads0.n
    if reads1.n != n:
        raise ValueError("the two read batches differ in length")
    res = np.ascontiguousarray(results, dtype=PAIR_RESULT_DTYPE)
    if res.shape != (n,) or len(cigars.editDistance) != 2 * n:
        raise ValueError("results / cigars do not have one entry per pair / two rows per pair")
    ed = np.ascontiguousarray(cigars.editDistance, dtype=np.int32)
    nops = np.ascontiguousarray(cigars.nOps, dtype=np.uint32)
    ops = np.ascontiguousarray(cigars.ops, dtype=np.uint32)
    rg = None if read_group is None else (read_group.encode() if isinstance(read_group, str) else bytes(read_group))
    keep = (res, ed, nops, ops, rg)
    ptr = lambda a: a.ctypes.data if a.size else None
    args = [index._h, reads0._p, reads1._p, ptr(res), ptr(ed), ptr(nops), ptr(ops), rg]
    ids = sum(int(np.ctypeslib.as_array(r._p.contents.idLengths, shape=(n,)).sum())
              for r in (reads0, reads1) if n and r._p.contents.idLengths)
    cap = ids + 2 * int(reads0._p.contents.totalBytes + reads1._p.contents.totalBytes) + 2 * n * 512
    return args, keep, cap


def _sized_call(fn, args, cap, what):
    """fn(*args, out, cap, &used) under the formatters' size contract -> bytes."""
    used = C.c_uint64()
    buf = np.empty(max(1, cap), dtype=np.uint8)
    rc = fn(*args, buf.ctypes.data, cap, C.byref(used))
    if rc != 0 and used.value > cap:
        cap = used.value
        buf = np.empty(cap, dtype=np.uint8)
        rc = fn(*args, buf.ctypes.data, cap, C.byref(used))
    _check(rc, what)
    return buf[:used.value].tobytes()


def sam_format_pairs(index, reads0, reads1, results, cigars, read_group="FASTQ", timing=None):
    """The two SAM lines of every pair (snapgpu_sam_format_pairs: SimpleReadWriter::writePair over
    SAMFormat::writeRead with a mate) -> bytes.  results: PAIR_RESULT_DTYPE records; cigars: 2n rows,
    row 2q + e for end e of pair q; the batches' own ids and clip state are used.  timing: a dict
    that receives the seconds spent in the C formatter ("format_s")."""
    args, keep, cap = _pair_inputs(index, reads0, reads1, results, cigars, read_group)
    t0 = time.perf_counter()
    text = _sized_call(lib().snapgpu_sam_format_pairs, args, cap, "sam_format_pairs")
    if timing is not None:
        timing["format_s"] = time.perf_counter() - t0
    return text


def sam_pair_line_lengths(index, reads0, reads1, results, cigars, read_group="FASTQ"):
    """Byte length of each of the 2n lines sam_format_pairs prints (the host side of the device
    formatter's length pass; needs no GPU) -> np.uint32 array."""
    args, keep, _ = _pair_inputs(index, reads0, reads1, results, cigars, read_group)
    out = np.zeros(max(1, 2 * reads0.n), dtype=np.uint32)
    _check(lib().snapgpu_sam_pair_line_lengths(*args, out.ctypes.data), "sam_pair_line_lengths")
    return out[:2 * reads0.n]


def _sam_pair_line_write(index, reads0, reads1, results, cigars, read_group="FASTQ"):
    """The same lines through csrc/sam_pair_line.h's writer on one host thread, the code the device
    write pass runs per wave (test accessor; needs no GPU)."""
    args, keep, cap = _pair_inputs(index, reads0, reads1, results, cigars, read_group)
    fn = lib().snapgpu_internal_sam_pair_line_write
    fn.restype = C.c_int
    fn.argtypes = _ffi._PAIR_LINES + [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    return _sized_call(fn, args, cap, "sam_pair_line_write")


def _pair_cigar_inputs(results):
    """(locations, directions) of the 2n CIGAR rows of pair records, row 2q + e: location[e], or
    invalid where status[e] is NotFound, and direction[e] (BaseAligner.Cigars' arguments)."""
    res = np.ascontiguousarray(results, dtype=PAIR_RESULT_DTYPE)
    loc = np.where(res["status"] != NotFound, res["location"], 0xFFFFFFFF).astype(np.uint32).reshape(-1)
    return np.ascontiguousarray(loc), np.ascontiguousarray(res["direction"].reshape(-1), dtype=np.uint8)


def _pair_cigars(aligner, reads0, reads1, results, useM=False):
    """The 2n CIGAR rows of pair records through the existing batch call (BaseAligner.Cigars on each
    end's batch at _pair_cigar_inputs' locations and directions), row 2q + e -> Cigars."""
    loc, dr = _pair_cigar_inputs(results)
    n = reads0.n
    c = Cigars.empty(2 * n)
    for e, r in enumerate((reads0, reads1)):
        k = aligner.Cigars(r, loc[e::2], dr[e::2], useM=useM)
        c.editDistance[e::2], c.nOps[e::2], c.ops[e::2] = k.editDistance, k.nOps, k.ops
    return c


def _carry_call(fn, args, nm_carry, cap, what, tail=()):
    """fn(*args, nm_carry, &carry, out, cap, &used, *tail) under the encoders' size contract ->
    (bytes, NM carry-out)."""
    used, carry = C.c_uint64(), C.c_int32()
    buf = np.empty(max(1, cap), dtype=np.uint8)
    rc = fn(*args, int(nm_carry), C.byref(carry), buf.ctypes.data, cap, C.byref(used), *tail)
    if rc != 0 and used.value > cap:
        cap = used.value
        buf = np.empty(cap, dtype=np.uint8)
        rc = fn(*args, int(nm_carry), C.byref(carry), buf.ctypes.data, cap, C.byref(used), *tail)
    _check(rc, what)
    return buf[:used.value].tobytes(), carry.value


def bam_format_pairs(index, reads0, reads1, results, cigars, read_group="FASTQ", nm_carry=0, timing=None):
    """The two uncompressed BAM records of every pair (snapgpu_bam_format_pairs:
    SimpleReadWriter::writePair over BAMFormat::writeRead with a mate), in write order -> (bytes, NM
    carry-out).  Arguments as sam_format_pairs; nm_carry: the NM that ends without location repeat
    until the first end with one.  timing: a dict that receives "format_s"."""
    args, keep, cap = _pair_inputs(index, reads0, reads1, results, cigars, read_group)
    t0 = time.perf_counter()
    out = _carry_call(lib().snapgpu_bam_format_pairs, args, nm_carry, cap, "bam_format_pairs")
    if timing is not None:
        timing["format_s"] = time.perf_counter() - t0
    return out


def _bam_append_pair_records(index, reads0, reads1, results, cigars, read_group="FASTQ", nm_carry=0):
    """bam_format_pairs' records through the RNA paired path's own encoder (bamAppendRecord with a
    mate, csrc/host/bam.cpp) on one host thread -> (bytes, NM carry-out) (tests)."""
    args, keep, cap = _pair_inputs(index, reads0, reads1, results, cigars, read_group)
    fn = lib().snapgpu_internal_bam_append_pair_records
    fn.restype = C.c_int
    fn.argtypes = _ffi._PAIR_RECORDS
    return _carry_call(fn, args, nm_carry, cap, "bam_append_pair_records")


def bam_pair_record_lengths(index, reads0, reads1, results, cigars, read_group="FASTQ"):
    """Byte size of each of the 2n records bam_format_pairs writes, block_size + 4 -> np.uint32 array."""
    args, keep, _ = _pair_inputs(index, reads0, reads1, results, cigars, read_group)
    out = np.zeros(max(1, 2 * reads0.n), dtype=np.uint32)
    _check(lib().snapgpu_bam_pair_record_lengths(*args, out.ctypes.data), "bam_pair_record_lengths")
    return out[:2 * reads0.n]


def bam_pair_sort_keys(index, results):
    """The coordinate-sort key of each of the 2n records of pair results, in write order
    (snapgpu_bam_pair_sort_keys: BAMFormat::getSortInfo, by piece index) -> np.uint32 array.
    np.argsort(keys, kind="stable") is the order of the sorted device calls."""
    res = np.ascontiguousarray(results, dtype=PAIR_RESULT_DTYPE)
    n = len(res)
    out = np.zeros(max(1, 2 * n), dtype=np.uint32)
    src = res if n else np.zeros(1, dtype=PAIR_RESULT_DTYPE)
    _check(lib().snapgpu_bam_pair_sort_keys(index._h, n, src.ctypes.data, out.ctypes.data), "bam_pair_sort_keys")
    return out[:2 * n]


def sam_sort_keys(index, results):
    """The coordinate-sort key of every record (snapgpu_sam_sort_keys: the host side of the sorted
    device formatter; needs no GPU) -> np.uint32 array.  np.argsort(keys, kind="stable") is the order
    of the sorted device calls and of sam_sort_records."""
    res = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
    n = len(res)
    out = np.zeros(max(1, n), dtype=np.uint32)
    src = res if n else np.zeros(1, dtype=RESULT_DTYPE)
    _check(lib().snapgpu_sam_sort_keys(index._h, n, src.ctypes.data, out.ctypes.data), "sam_sort_keys")
    return out[:n]


def bam_format(index, reads, ids, results, cigars, read_group="FASTQ", clip=None, nm_carry=0):
    """Uncompressed BAM records (BAMFormat::writeRead, Bam.cpp:596-790) of single-end genome
    alignments, in input order -> (bytes, NM carry-out).  Arguments as sam_format; nm_carry: the NM
    that records without CIGAR ops repeat until the first record with ops (snapgpu_bam_format)."""
    args, keep, cap = _sam_inputs(reads, ids, results, cigars, read_group, clip)
    used, carry = C.c_uint64(), C.c_int32()
    buf = np.empty(max(1, cap), dtype=np.uint8)
    fn = lib().snapgpu_bam_format
    rc = fn(index._h, *args, int(nm_carry), C.byref(carry), buf.ctypes.data, cap, C.byref(used))
    if rc != 0 and used.value > cap:
        buf = np.empty(used.value, dtype=np.uint8)
        rc = fn(index._h, *args, int(nm_carry), C.byref(carry), buf.ctypes.data, used.value, C.byref(used))
    _check(rc, "bam_format")
    return buf[:used.value].tobytes(), carry.value


def _bam_append_records(index, reads, ids, results, cigars, read_group="FASTQ", clip=None, nm_carry=0):
    """bam_format's records through the product paths' own encoder (bamAppendRecord, csrc/host/bam.cpp)
    on one host thread -> (bytes, NM carry-out) (tests)."""
    args, keep, cap = _sam_inputs(reads, ids, results, cigars, read_group, clip)
    used, carry = C.c_uint64(), C.c_int32()
    buf = np.empty(max(1, cap), dtype=np.uint8)
    fn = lib().snapgpu_internal_bam_append_records
    fn.restype = C.c_int
    fn.argtypes = ([C.c_void_p, C.POINTER(_ffi.Reads), C.c_char_p] + [C.c_void_p] * 6 + [C.c_char_p] + [C.c_void_p] * 2 +
                   [C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)])
    rc = fn(index._h, *args, int(nm_carry), C.byref(carry), buf.ctypes.data, cap, C.byref(used))
    if rc != 0 and used.value > cap:
        buf = np.empty(used.value, dtype=np.uint8)
        rc = fn(index._h, *args, int(nm_carry), C.byref(carry), buf.ctypes.data, used.value, C.byref(used))
    _check(rc, "bam_append_records")
    return buf[:used.value].tobytes(), carry.value


def bam_record_lengths(index, reads, ids, results, cigars, read_group="FASTQ", clip=None):
    """Byte size of every record bam_format writes, block_size + 4 (snapgpu_bam_record_lengths: the
    host side of the device encoder's length pass) -> np.uint32 array."""
    args, keep, _ = _sam_inputs(reads, ids, results, cigars, read_group, clip)
    out = np.zeros(max(1, reads.n), dtype=np.uint32)
    _check(lib().snapgpu_bam_record_lengths(index._h, *args, out.ctypes.data), "bam_record_lengths")
    return out[:reads.n]


def bam_sort_keys(index, results):
    """The coordinate-sort key of every BAM record (snapgpu_bam_sort_keys: BAMFormat::getSortInfo, by
    piece index) -> np.uint32 array.  np.argsort(keys, kind="stable") is the order of the sorted
    device calls."""
    res = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
    n = len(res)
    out = np.zeros(max(1, n), dtype=np.uint32)
    src = res if n else np.zeros(1, dtype=RESULT_DTYPE)
    _check(lib().snapgpu_bam_sort_keys(index._h, n, src.ctypes.data, out.ctypes.data), "bam_sort_keys")
    return out[:n]


def bam_header(index, sam_header_text):
    """The BAM header (BAMFormat::writeHeader, Bam.cpp:542-594) around a SAM header text -> bytes."""
    text = sam_header_text.encode() if isinstance(sam_header_text, str) else bytes(sam_header_text)
    used = C.c_uint64()
    lib().snapgpu_bam_header(index._h, text, len(text), None, 0, C.byref(used))
    buf = C.create_string_buffer(max(1, used.value))
    _check(lib().snapgpu_bam_header(index._h, text, len(text), buf, used.value, C.byref(used)), "bam_header")
    return C.string_at(buf, used.value)


def bgzf_compress(data, eof=True):
    """BGZF blocks of `data` (0xff00 input bytes each, compressed on the host threads), then the EOF
    block if eof (snapgpu_bgzf_compress) -> bytes.  gzip.decompress gives `data` back."""
    src = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    n = int(src.size)
    cap = n + (n // 0xff00 + 1) * 128 + 256
    buf = np.empty(cap, dtype=np.uint8)
    used = C.c_uint64()
    _check(lib().snapgpu_bgzf_compress(src.ctypes.data if n else None, n, int(bool(eof)), buf.ctypes.data, cap,
                                       C.byref(used)), "bgzf_compress")
    return buf[:used.value].tobytes()


def bai_build(records, bgzf, n_ref, stream_offset=0):
    """The .bai index of the coordinate-sorted BAM records `records` and a BGZF stream `bgzf` of them
    (bgzf_compress's, bgzf_compress_model's or the device's; with or without the EOF block) -> bytes.
    stream_offset: the compressed bytes ahead of that stream in the file.  The host model of the device
    index (snapgpu_bai_build; needs no GPU)."""
    rec = np.frombuffer(bytes(records), dtype=np.uint8)
    z = np.frombuffer(bytes(bgzf), dtype=np.uint8)
    fn = lib().snapgpu_bai_build
    args = (rec.ctypes.data if rec.size else None, int(rec.size), int(n_ref), z.ctypes.data if z.size else None,
            int(z.size), int(stream_offset))
    used = C.c_uint64()
    rc = fn(*args, None, 0, C.byref(used))
    if rc != 0 and used.value == 0:
        _check(rc, "bai_build")
    buf = np.empty(max(1, used.value), dtype=np.uint8)
    _check(fn(*args, buf.ctypes.data, used.value, C.byref(used)), "bai_build")
    return buf[:used.value].tobytes()


def bam_mark_duplicates(records, n_ref):
    """(records with FLAG 0x400 on the duplicates, n_marked, n_groups) of the coordinate-sorted single-end
    BAM records `records`: the host model of the device marking (snapgpu_bam_mark_duplicates; needs no
    GPU).  n_groups counts the groups of two or more."""
    buf = np.frombuffer(bytes(records), dtype=np.uint8).copy()
    marked, groups = C.c_uint64(), C.c_uint64()
    _check(lib().snapgpu_bam_mark_duplicates(buf.ctypes.data if buf.size else None, int(buf.size), int(n_ref),
                                             C.byref(marked), C.byref(groups)), "bam_mark_duplicates")
    return buf.tobytes(), marked.value, groups.value


def write_sorted_bam(path, index, sam_header_text, dev, mark_duplicates=False):
    """Write the coordinate-sorted BGZF BAM `path` and its index `path + ".bai"` from a resident batch
    after run_bam(sorted_output=True): the BAM header compressed on the host (no EOF block), then
    run_bgzf()'s members and the EOF block; the index is run_bai()'s, with the header's compressed
    bytes as its stream offset.  mark_duplicates: run_dupmark() ahead of the compressor, so that the
    file's records carry FLAG 0x400 on the duplicates."""
    head = bgzf_compress(bam_header(index, sam_header_text), eof=False)
    if mark_duplicates:
        dev.run_dupmark()
    dev.run_bgzf()
    dev.run_bai(stream_offset=len(head))
    body, bai = dev.bgzf(), dev.bai()
    with open(path, "wb") as f:
        f.write(head)
        f.write(body)
    with open(path + ".bai", "wb") as f:
        f.write(bai)


def _bgzf_call(fn, data, eof, what):
    """fn(in, n, eof, out, cap, used) of the device compressor or its host model over `data` -> bytes.
    A member takes at most its input + 31 bytes."""
    src = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    n = int(src.size)
    cap = n + (n // 0xff00 + 1) * 31 + 28
    buf = np.empty(cap, dtype=np.uint8)
    used = C.c_uint64()
    _check(fn(src.ctypes.data if n else None, n, int(bool(eof)), buf.ctypes.data, cap, C.byref(used)), what)
    return buf[:used.value].tobytes()


def bgzf_compress_model(data, eof=True):
    """The device BGZF compressor's stream from the host threads, byte for byte (snapgpu_bgzf_compress_model:
    the serial restatement of csrc/bgzf_block.h; needs no GPU) -> bytes.  gzip.decompress gives `data` back."""
    return _bgzf_call(lib().snapgpu_bgzf_compress_model, data, eof, "bgzf_compress_model")


def bgzf_inflate_size(data):
    """(bytes the BGZF stream `data` inflates to, its members): the member walk alone
    (snapgpu_bgzf_inflate_size).  Raises for a stream that is not BGZF."""
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    out, members = C.c_uint64(), C.c_uint64()
    _check(lib().snapgpu_bgzf_inflate_size(src.ctypes.data if src.size else None, int(src.size), C.byref(out),
                                           C.byref(members)), "bgzf_inflate_size")
    return out.value, members.value


def _inflate_call(fn, data, what):
    """fn(in, n, out, cap, used) of an inflater over the BGZF stream `data` -> bytes: a first call for
    the size (the size contract of include/snapgpu.h), a second into a buffer of it."""
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    n = int(src.size)
    size, _ = bgzf_inflate_size(data)
    buf = np.empty(max(1, size), dtype=np.uint8)
    used = C.c_uint64()
    _check(fn(src.ctypes.data if n else None, n, buf.ctypes.data, size, C.byref(used)), what)
    return buf[:used.value].tobytes()


def bgzf_inflate(data):
    """The bytes of the BGZF stream `data`, inflated by zlib on the host threads (snapgpu_bgzf_inflate:
    bgzf_compress's counterpart).  gzip.decompress gives the same bytes."""
    return _inflate_call(lib().snapgpu_bgzf_inflate, data, "bgzf_inflate")


def bgzf_inflate_model(data):
    """The same through csrc/inflate_block.h on the host threads, the decoder the device kernel
    compiles (snapgpu_bgzf_inflate_model; needs no GPU and no zlib)."""
    return _inflate_call(lib().snapgpu_bgzf_inflate_model, data, "bgzf_inflate_model")


def _sam_line_write(index, reads, ids, results, cigars, read_group="FASTQ", clip=None):
    """The device write pass's line writer (csrc/sam_line.h) run on one host thread -> bytes (tests)."""
    args, keep, _ = _sam_inputs(reads, ids, results, cigars, read_group, clip)
    total = int(sam_line_lengths(index, reads, ids, results, cigars, read_group, clip).sum(dtype=np.uint64))
    buf = np.empty(max(1, total), dtype=np.uint8)
    fn = lib().snapgpu_internal_sam_line_write
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(_ffi.Reads), C.c_char_p] + [C.c_void_p] * 6 + [C.c_char_p] + [C.c_void_p] * 3
    _check(fn(index._h, *args, buf.ctypes.data), "sam_line_write")
    return buf[:total].tobytes()


LV_PASS_GROUPS = 8      # SNAPGPU_LV_PASS_GROUPS: lane groups of a pass at the smallest group size
LV_MAX_K = 31           # LandauVishkin.h MAX_K
FRES_VALID = 1 << 31    # snapgpu_lv_filter_batch: the task's window was servable


def lv_group_size(k):
    """Lanes per candidate of a scoring pass at limit k (score_batched's choice)."""
    k = min(k, LV_MAX_K - 1)
    return 8 if k <= 3 else 16 if k <= 7 else 32 if k <= 15 else 64


def lv_pass_batch(passes, device=0, nw=None):
    """Scoring passes as align_kernel<128> / <256> run them (snapgpu_lv_pass_batch): one wave per pass.

    passes: list of dicts {read, quals, seedLen, k, cands}; cands lists the pass's lane groups in order, each
    None (no candidate) or a dict {genome, before, dir, s, act, glen[, rtl]}: `genome` holds the candidate's
    bytes, position 0 at offset `before`.  nw: 64-bit mask words (2 or 4; default 4 when a read is longer than
    128 bases).  -> per pass, per group: (e1, e2, p1, p2, netIndel)."""
    n = len(passes)
    if nw is None:
        nw = 4 if any(len(p["read"]) > 128 for p in passes) else 2
    reads, quals, genome = bytearray(), bytearray(), bytearray()
    roff, rlen, sl, ks = [], [], [], []
    cand = np.zeros((max(1, n), LV_PASS_GROUPS, 8), dtype=np.int64)
    for i, p in enumerate(passes):
        r = p["read"].encode() if isinstance(p["read"], str) else bytes(p["read"])
        q = p["quals"].encode() if isinstance(p["quals"], str) else bytes(p["quals"])
        roff.append(len(reads)); rlen.append(len(r)); reads += r; quals += q[:len(r)].ljust(len(r), b"!")
        sl.append(p["seedLen"]); ks.append(p["k"])
        if len(p["cands"]) > LV_PASS_GROUPS:
            raise ValueError("more candidates than lane groups")
        for g, c in enumerate(p["cands"]):
            if c is None:
                continue
            gb = c["genome"].encode() if isinstance(c["genome"], str) else bytes(c["genome"])
            cand[i, g] = (len(genome) + c["before"], c["before"], len(gb) - c["before"], c["dir"], c["s"],
                          1 if c["act"] else 0, c["glen"], c.get("rtl", c["s"] + LV_MAX_K))
            genome += gb
    reads += b"\0" * 16; quals += b"\0" * 16; genome += b"\0" * 16
    A64, A32, AI = C.c_uint64 * n, C.c_uint32 * n, C.c_int32 * n
    no = max(1, n) * LV_PASS_GROUPS
    e1, e2, net = (C.c_int32 * no)(), (C.c_int32 * no)(), (C.c_int32 * no)()
    p1, p2 = (C.c_double * no)(), (C.c_double * no)()
    _check(lib().snapgpu_lv_pass_batch(device, nw, n, bytes(reads), bytes(quals), len(reads) - 16, A64(*roff),
                                       A32(*rlen), AI(*sl), AI(*ks), bytes(genome), len(genome) - 16,
                                       cand.ctypes.data_as(C.POINTER(C.c_int64)), e1, e2, p1, p2, net), "lv_pass_batch")
    return [[(e1[j], e2[j], p1[j], p2[j], net[j]) for j in range(i * LV_PASS_GROUPS, i * LV_PASS_GROUPS + len(p["cands"]))]
            for i, p in enumerate(passes)]


def lv_filter_batch(aligner, quad, tasks):
    """The forced-mode prefilter on explicit tasks (snapgpu_lv_filter_batch) over `aligner`'s device genome.

    tasks: list of (read, loc, dir, s, k, act); quad False: lane pairs (k <= 5), True: lane quads (k <= 7).
    -> uint32 array of encoded results (0, or FRES_VALID | e1 << 8 | e2 << 11; 7 = above the limit)."""
    n = len(tasks)
    reads = bytearray()
    roff, rlen = [], []
    for t in tasks:
        r = t[0].encode() if isinstance(t[0], str) else bytes(t[0])
        roff.append(len(reads)); rlen.append(len(r)); reads += r
    reads += b"\0" * 16
    A64, A32, AI = C.c_uint64 * n, C.c_uint32 * n, C.c_int32 * n
    out = np.zeros(max(1, n), dtype=np.uint32)
    _check(lib().snapgpu_lv_filter_batch(aligner._h, 1 if quad else 0, n, bytes(reads), len(reads) - 16, A64(*roff),
                                         A32(*rlen), A32(*[t[1] for t in tasks]), AI(*[t[2] for t in tasks]),
                                         AI(*[t[3] for t in tasks]), AI(*[t[4] for t in tasks]),
                                         AI(*[1 if t[5] else 0 for t in tasks]),
                                         out.ctypes.data_as(C.POINTER(C.c_uint32))), "lv_filter_batch")
    return out[:n]


def _lv_batch_bitplane(direction, tasks, device):
    """LV tasks as scoring passes (lv_pass_batch): task i sits in lane group i % (64 / GS) of its own pass,
    the other groups inactive.  A forward task is a read with an empty seed at offset 0 (the forward call
    scores the whole read against the text); a reverse task is the reversed pattern as a read whose empty
    seed sits at its end (the reverse call scores it backwards against the text's end).  Texts are padded
    with 'n' as the reference harness pads them."""
    PAD = 64
    passes, where = [], []
    for i, (t, p, q, k) in enumerate(tasks):
        t = t.encode() if isinstance(t, str) else bytes(t)
        p = p.encode() if isinstance(p, str) else bytes(p)
        q = (q.encode() if isinstance(q, str) else bytes(q))[:len(p)].ljust(len(p), b"!")
        pl, tl = len(p), len(t)
        g = i % (64 // lv_group_size(k))
        gen = b"n" * PAD + t + b"n" * PAD
        if direction > 0:
            c = dict(genome=gen, before=PAD, dir=0, s=0, act=1, glen=tl)
            ps = dict(read=p, quals=q, seedLen=0, k=k)
        else:   # genome[y] = text[tl - pl + y]; the forward call sees an empty pattern
            c = dict(genome=gen, before=PAD + tl - pl, dir=0, s=pl, act=1, glen=pl, rtl=tl)
            ps = dict(read=p[::-1], quals=q[::-1], seedLen=0, k=k)
        ps["cands"] = [None] * g + [c]
        passes.append(ps)
        where.append(g)
    nw = 4 if any(len(ps["read"]) > 127 for ps in passes) else 2
    out = []
    for ps, g, r in zip(passes, where, lv_pass_batch(passes, device, nw)):
        e1, e2, p1, p2, net = r[g]
        if direction > 0:
            out.append((e1, 0, p1 if e1 >= 0 else 1.0))
        else:
            out.append((e2, net if e2 >= 0 else 0, p2 if e2 >= 0 else 1.0))
    return out


def lv_batch(direction, tasks, device=0, engine="byte"):
    """LandauVishkin<direction>::computeEditDistance on the GPU.

    tasks: list of (text, pattern, quals, k) (str/bytes).  -> list of (score, netIndel, prob).
    engine "byte": the byte-compare LV of align_kernel<512>; "bitplane": the production LV of
    align_kernel<128> / <256> through the pass kernel (patterns of 1..253 bases; any pattern longer than
    127 bases puts the batch on 256-bit masks; netIndel for direction -1 only)."""
    if engine != "byte":
        return _lv_batch_bitplane(direction, tasks, device)
    n = len(tasks)
    texts, pats, quals = bytearray(), bytearray(), bytearray()
    toff, tlen, poff, plen, ks = [], [], [], [], []
    for t, p, q, k in tasks:
        t = t.encode() if isinstance(t, str) else bytes(t)
        p = p.encode() if isinstance(p, str) else bytes(p)
        q = q.encode() if isinstance(q, str) else bytes(q)
        toff.append(len(texts)); tlen.append(len(t)); texts += t
        poff.append(len(pats)); plen.append(len(p)); pats += p; quals += q[:len(p)].ljust(len(p), b"!")
        ks.append(k)
    texts += b"\0" * 16; pats += b"\0" * 16; quals += b"\0" * 16
    A64, A32, AI = C.c_uint64 * n, C.c_uint32 * n, C.c_int32 * n
    os_, on, op = AI(), AI(), (C.c_double * n)()
    _check(lib().snapgpu_lv_batch(device, direction, n, bytes(texts), A64(*toff), A32(*tlen), bytes(pats),
                                  bytes(quals), A64(*poff), A32(*plen), AI(*ks), os_, on, op), "lv_batch")
    return [(os_[i], on[i], op[i]) for i in range(n)]


def compute_mapq(pAll, pBest, score, popularSeedsSkipped):
    return lib().snapgpu_compute_mapq(pAll, pBest, score, popularSeedsSkipped)


class Gtf:
    """Genome annotation (SNAPLib/GTFReader: exon lines -> transcripts with introns)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load(cls, path):
        return cls(_check(lib().snapgpu_gtf_load(str(path).encode()), "gtf_load"))

    def counts(self):
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib().snapgpu_gtf_counts(self._h, C.byref(a), C.byref(b), C.byref(c)), "gtf_counts")
        return {"features": a.value, "transcripts": b.value, "genes": c.value}

    def write_transcriptome(self, genome, path):
        """GTFReader::BuildTranscriptome: the transcriptome FASTA `snap-rna transcriptome` indexes.
        genome: a Genome or a raw genome handle (GenomeIndex.genome_handle())."""
        g = genome._h if isinstance(genome, Genome) else genome
        _check(lib().snapgpu_gtf_write_transcriptome(self._h, g, str(path).encode()), "gtf_write_transcriptome")

    def genomic_position(self, transcript_id, pos, span):
        out = C.c_uint32()
        _check(lib().snapgpu_gtf_genomic_position(self._h, transcript_id.encode(), pos, span, C.byref(out)),
               "gtf_genomic_position")
        return out.value

    def splice_cigar(self, transcript_id, pos, tokens):
        """insertSpliceJunctions over [(count, op), ...] -> CIGAR string."""
        counts = (C.c_uint32 * max(1, len(tokens)))(*[int(c) for c, _ in tokens])
        ops = "".join(o for _, o in tokens).encode()
        used = C.c_uint64()
        buf = C.create_string_buffer(4096)
        _check(lib().snapgpu_gtf_splice_cigar(self._h, transcript_id.encode(), pos, len(tokens), counts, ops, buf,
                                              4096, C.byref(used)), "gtf_splice_cigar")
        return buf.value.decode()

    def write_counts(self, prefix):
        """GTFReader::WriteReadCounts: <prefix>.{transcript,gene,junction}_{id,name}.counts.txt."""
        _check(lib().snapgpu_gtf_write_counts(self._h, str(prefix).encode()), "gtf_write_counts")

    def reset_counts(self):
        _check(lib().snapgpu_gtf_reset_counts(self._h), "gtf_reset_counts")

    def __del__(self):
        if getattr(self, "_h", None):
            lib().snapgpu_gtf_free(self._h)
            self._h = None


def sam_sort_records(index, text):
    """`-so`: SAM record lines (bytes, no header) stable-sorted by SAMFormat::getSortInfo's location."""
    used = C.c_uint64()
    buf = C.create_string_buffer(max(1, len(text)))
    _check(lib().snapgpu_sam_sort_records(index._h, text, len(text), buf, len(text), C.byref(used)), "sam_sort_records")
    return C.string_at(buf, used.value)


class Contaminants:
    """The contamination database's counts (`-ct`, ContaminationFilter): contaminant alignments per
    contig of the contamination index, accumulated over the product-path calls given
    contamination=(aligner, this); write() leaves `<prefix>.contaminants.txt` as the reference."""

    def __init__(self, contamination_index):
        self._index = contamination_index
        self._h = _check(lib().snapgpu_contaminants_create(contamination_index._h), "contaminants_create")

    def add(self, location):
        """ContaminationFilter::AddAlignment of one aligned location of the contamination genome."""
        _check(lib().snapgpu_contaminants_add(self._h, int(location)), "contaminants_add")

    def text(self):
        used = C.c_uint64()
        _check(lib().snapgpu_contaminants_format(self._h, None, 0, C.byref(used)), "contaminants_format")
        buf = C.create_string_buffer(max(1, used.value))
        _check(lib().snapgpu_contaminants_format(self._h, buf, used.value, C.byref(used)), "contaminants_format")
        return C.string_at(buf, used.value).decode()

    def write(self, output_template):
        _check(lib().snapgpu_contaminants_write(self._h, None if output_template is None else str(output_template).encode()),
               "contaminants_write")

    def __del__(self):
        if getattr(self, "_h", None):
            lib().snapgpu_contaminants_free(self._h)
            self._h = None


def _contamination_opts(o, contamination):
    if contamination is not None:
        aligner, counts = contamination
        o.contaminationAligner = aligner._h
        o.contaminants = counts._h


def single_options(**kw):
    o = _ffi.SingleOptions()
    lib().snapgpu_single_options_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v.encode() if isinstance(v, str) else v)
    return o


def single_align(genome_aligner, transcriptome_aligner, gtf, reads, sam_path, contamination=None, **options):
    """`snap-rna single` (SingleAligner.cpp:141-320) over a FASTQ batch, both AlignRead calls and
    the CIGARs on the GPU; writes sam_path.  options: SingleOptions fields; contamination:
    (BaseAligner over the contamination index, Contaminants) for `-ct`.  -> stats dict."""
    o = single_options(**options)
    _contamination_opts(o, contamination)
    st = _ffi.SingleStats()
    _check(lib().snapgpu_single_align(genome_aligner._h, transcriptome_aligner._h, gtf._h, reads._p, C.byref(o),
                                      str(sam_path).encode(), C.byref(st)), "single_align")
    return {f: getattr(st, f) for f, _ in st._fields_}


RNA_PAIR_RESULT_DTYPE = np.dtype([
    ("location", "<u4", (2,)), ("tlocation", "<u4", (2,)), ("score", "<i4", (2,)), ("mapq", "<i4", (2,)),
    ("status", "u1", (2,)), ("direction", "u1", (2,)), ("isTranscriptome", "u1", (2,)), ("fromAlignTogether", "u1"),
    ("alignedAsPair", "u1"), ("useful", "u1"), ("reserved", "u1", (7,)),
])
assert RNA_PAIR_RESULT_DTYPE.itemsize == 48


def rna_paired_options(**kw):
    o = _ffi.RnaPairedOptions()
    lib().snapgpu_rna_paired_options_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v.encode() if isinstance(v, str) else v)
    return o


def rna_paired_align(paired_aligner, transcriptome_aligner, gtf, reads0, reads1, sam_path=None, contamination=None,
                     **options):
    """`snap-rna paired` (PairedAligner.cpp:405-689) over a FASTQ pair batch: the transcriptome and
    genome aligners, the seed census of FindPartialMatches and the CIGARs on the GPU; writes
    sam_path (if given) and advances gtf's read counters.  -> (RNA_PAIR_RESULT_DTYPE[n], stats)."""
    o = rna_paired_options(**options)
    _contamination_opts(o, contamination)   # (PairedAligner over the contamination index, Contaminants): -ct
    st = _ffi.RnaPairedStats()
    out = np.zeros(max(1, reads0.n), dtype=RNA_PAIR_RESULT_DTYPE)
    _check(lib().snapgpu_rna_paired_align(paired_aligner._h, transcriptome_aligner._h, gtf._h, reads0._p, reads1._p,
                                          C.byref(o), None if sam_path is None else str(sam_path).encode(),
                                          out.ctypes.data, C.byref(st)), "rna_paired_align")
    return out[:reads0.n], {f: getattr(st, f) for f, _ in st._fields_}
