/*
 * snapgpu.h -- C ABI of the MI355X-native SNAP seed-and-extend hot path.
 *
 * This is the drop-in boundary for SNAPLib's `Aligner` / `BaseAligner` surface
 * (reference: SNAPLib/Aligner.h:54-80, SNAPLib/BaseAligner.h:44-142).  Every entry
 * point is plain C (pointers + sizes, no C++ or torch types) so that the
 * reference's C++ (apps/snap, SingleAlignerContext via AlignerExtension,
 * SNAPLib/AlignerContext.h:132-163) -- or ctypes / any FFI -- can bind it.
 * INTEGRATION.md shows the adapter a SNAPLib maintainer would add.
 *
 * Conventions
 *  - Functions returning int return SNAPGPU_OK (0) on success, a negative
 *    SNAPGPU_E* code on failure; snapgpu_last_error() gives the message.  The
 *    reference calls soft_exit() (SNAPLib/exit.cpp:27-31) where this API returns
 *    an error code instead (e.g. a read longer than maxReadSize,
 *    BaseAligner.cpp:609-613 -> per-read flag SNAPGPU_FLAG_READ_TOO_LONG).
 *  - Handles are opaque; an aligner handle is bound to one GPU and must be used
 *    from one host thread at a time (the reference's BaseAligner is likewise not
 *    thread safe, Aligner.h:19-20).
 *  - Genome locations are the reference's 0-based offsets into the padded
 *    whole-genome string (Genome.h:29, FASTA.cpp:67-125).
 */
#ifndef SNAPGPU_H
#define SNAPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: snapgpu_timing_t.nNulReads / nUnwritten, SNAPGPU_FLAG_NUL_BYTE, SNAPGPU_PFLAG_NUL_BYTE, the
 *    buffer length of snapgpu_phase_cycles */
#define SNAPGPU_ABI_VERSION 2

enum {
    SNAPGPU_OK = 0,
    SNAPGPU_EINVAL = -1,      /* bad argument */
    SNAPGPU_EIO = -2,         /* file could not be read/written */
    SNAPGPU_ENOMEM = -3,      /* host or device allocation failed */
    SNAPGPU_EDEVICE = -4,     /* HIP runtime error / no GPU */
    SNAPGPU_EFORMAT = -5,     /* index/genome file format error */
    SNAPGPU_EUNSUPPORTED = -6 /* parameter combination not supported */
};

/* AlignmentResult (SNAPLib/Read.h:41) */
enum { SNAPGPU_NOT_FOUND = 0, SNAPGPU_SINGLE_HIT = 1, SNAPGPU_MULTIPLE_HITS = 2, SNAPGPU_UNKNOWN = 3 };
/* Direction (SNAPLib/directions.h:26-35) */
enum { SNAPGPU_FORWARD = 0, SNAPGPU_RC = 1 };

/* per-read flags in snapgpu_result_t.flags */
#define SNAPGPU_FLAG_READ_TOO_LONG  0x01u  /* reference: soft_exit(1), BaseAligner.cpp:609-613 */
#define SNAPGPU_FLAG_MAPQ_FIXED     0x02u  /* MAPQ re-derived on host with libm log10 (boundary case) */
#define SNAPGPU_FLAG_DEFERRED       0x04u  /* left pass 1 (read > 128 bases, or IUPAC codes in both read and
                                              genome): aligned by align_kernel<256> or align_kernel<512> */
#define SNAPGPU_FLAG_TOO_MANY_NS    0x08u  /* countOfNs > maxK (BaseAligner.cpp:652-655) */
#define SNAPGPU_FLAG_BYTE_PATH      0x10u  /* aligned by the byte-compare pass 3, align_kernel<512> (read
                                              > 256 bases, or IUPAC codes in both read and genome) */
#define SNAPGPU_FLAG_NUL_BYTE       0x20u  /* the read holds a 0x00 byte inside its length: no FASTQ/SAM
                                              reader produces one, so it marks a corrupted or unfinished
                                              upload (the aligner still treats it as a non-ACGT base, as
                                              the reference would); counted in snapgpu_timing_t.nNulReads */

/*
 * Result of one AlignRead call (BaseAligner.cpp:510-938).  location / direction /
 * score / mapq are exactly what AlignRead writes through its out-pointers,
 * including the "written before the result is known" conventions
 * (BaseAligner.cpp:582-584, 1357-1360): location=0xffffffff, direction=FORWARD,
 * score=0xffff when nothing was scored.  mapq is 0 when AlignRead returns before
 * writing it (short read / too many Ns).  The remaining fields are the per-read
 * deltas of BaseAligner's statistics getters (BaseAligner.h:113-117) and its
 * private MAPQ inputs (BaseAligner.h:284-285,333), exported for parity checking
 * and roofline accounting.
 */
typedef struct snapgpu_result {
    uint32_t location;
    int32_t  score;
    int32_t  mapq;
    uint8_t  result;      /* SNAPGPU_NOT_FOUND .. */
    uint8_t  direction;   /* SNAPGPU_FORWARD / SNAPGPU_RC */
    uint8_t  flags;       /* SNAPGPU_FLAG_* */
    uint8_t  reserved;
    uint32_t nLookups;            /* getNHashTableLookups() delta */
    uint32_t nLocationsScored;    /* getLocationsScored() delta */
    uint16_t popularSeedsSkipped; /* BaseAligner::popularSeedsSkipped */
    uint16_t nHitsIgnored;        /* getNHitsIgnoredBecauseOfTooHighPopularity() delta */
    uint32_t nProbes;             /* 64-B bucket lines of the seed-table image loaded (roofline P; device statistic) */
    uint32_t nHitWords;           /* hit words consumed (roofline H) */
    uint32_t nOverflowLists;      /* overflow lists visited (roofline V) */
    uint32_t nElements;           /* candidate elements allocated (BaseAligner.cpp:1485-1568) */
    uint32_t reserved2;
    double   probabilityOfAllCandidates;
    double   probabilityOfBestCandidate;
} snapgpu_result_t;   /* 64 bytes */

/* BaseAligner constructor parameters (BaseAligner.h:44-55, defaults of
 * AlignerOptions.cpp:33-85 / SingleAligner.cpp:167-179). */
typedef struct snapgpu_aligner_params {
    uint32_t maxHitsToConsider;  /* -h, default 300 */
    uint32_t maxK;               /* -d, default 14 */
    uint32_t maxReadSize;        /* MAX_READ_LENGTH (Read.h:45), default 500 */
    uint32_t maxSeedsToUse;      /* -n, default 25 (0 => use seedCoverage) */
    double   maxSeedCoverage;    /* -sc, used iff maxSeedsToUse == 0 */
    uint32_t extraSearchDepth;   /* default 2 */
    uint32_t explorePopularSeeds;/* setExplorePopularSeeds (BaseAligner.h:139) */
    uint32_t stopOnFirstHit;     /* setStopOnFirstHit (BaseAligner.h:142) */
} snapgpu_aligner_params_t;

void snapgpu_aligner_params_default(snapgpu_aligner_params_t *p);

/* ------------------------------------------------------------------ genome */
typedef struct snapgpu_genome snapgpu_genome_t;

/* ReadFASTAGenome (SNAPLib/FASTA.cpp:31-130): upper-cases, N -> 'n',
 * `chromosomePadding` 'n's before every contig and at the end. */
snapgpu_genome_t *snapgpu_genome_from_fasta(const char *path, uint32_t chromosomePadding);

/* Deterministic synthetic genome (no reference equivalent; stands in for
 * GRCh38 data that is not available offline).  See DESIGN.md "Synthetic data". */
typedef struct snapgpu_synth_genome_params {
    uint64_t seed;               /* PRNG seed (e.g. 2121) */
    uint64_t totalBases;         /* sum of contig lengths (excl. padding) */
    uint32_t nContigs;
    uint32_t nRepeatFamilies;    /* 0 => uniform random genome */
    double   repeatFraction;     /* target fraction of repeat-derived bases */
    double   maxDivergence;      /* per-copy divergence ~ U(0, maxDivergence) */
    double   nRunFraction;       /* fraction of bases in runs of N */
    uint32_t chromosomePadding;  /* default 500 */
} snapgpu_synth_genome_params_t;
snapgpu_genome_t *snapgpu_genome_synthetic(const snapgpu_synth_genome_params_t *p);
int  snapgpu_genome_write_fasta(const snapgpu_genome_t *g, const char *path);
void snapgpu_genome_free(snapgpu_genome_t *g);
uint32_t snapgpu_genome_nbases(const snapgpu_genome_t *g);
/* pointer to base 0 of the padded genome string; bytes [-256, nBases+256) are readable */
const char *snapgpu_genome_bases(const snapgpu_genome_t *g);
int snapgpu_genome_npieces(const snapgpu_genome_t *g);
uint32_t snapgpu_genome_piece_offset(const snapgpu_genome_t *g, int i);
const char *snapgpu_genome_piece_name(const snapgpu_genome_t *g, int i);

/* ------------------------------------------------------------------- index */
typedef struct snapgpu_index snapgpu_index_t;

/* GenomeIndex::BuildIndexToDirectory semantics (GenomeIndex.cpp:348-720): every
 * genome offset in [0, nBases - seedLen - 1) whose seedLen bases are all ACGT is
 * indexed under its canonical (smaller of seed / reverse complement) seed;
 * overflow lists are sorted descending (GenomeIndex.cpp:616-618).  The layout of
 * the SNAPHashTable slots differs from the reference's multi-threaded builder
 * (as it does between two reference builds), the lookup results do not.
 * Takes ownership of `genome`.  nThreads <= 0 => hardware concurrency. */
snapgpu_index_t *snapgpu_index_build(snapgpu_genome_t *genome, int seedLen, int nThreads);
/* As snapgpu_index_build with the table-size slack of `snap-rna index -h` (GenomeIndex.cpp:208,
 * default 0.3; <= 0 => 0.3): table i gets (nBases * (1 + slack) / nTables) * bias_i slots with the
 * exact bias of ComputeBiasTable (GenomeIndex.cpp:1109-1243, 294-346), at least 100 -- the
 * reference's load factor and probe chains. */
snapgpu_index_t *snapgpu_index_build_ex(snapgpu_genome_t *genome, int seedLen, int nThreads, double slack);
/* snapgpu_index_build_ex on HIP device `device`: seed scan, sort, run and overflow layout, hash
 * placement and the table image are computed in HBM and copied into a host index.  Identity
 * guarantee: slots, overflow, tableBase, tableSize, tableUsed, hasIupac and every
 * snapgpu_index_info_t field are byte-identical to what snapgpu_index_build_ex(genome, seedLen,
 * any nThreads, slack) returns, so the result serves save, share, lookup, get_view, every aligner
 * and the oracle alike.  Same contract: takes ownership of `genome`, seedLen 16..31, slack <= 0
 * => 0.3.  NULL (genome freed, snapgpu_last_error set) on a bad device or seedLen, on too little
 * free device memory (asked of hipMemGetInfo before allocating; the message names SNAPGPU_ENOMEM,
 * the bytes needed and the bytes free) and on any HIP error.  There is no fallback to the CPU
 * builder. */
snapgpu_index_t *snapgpu_index_build_gpu(snapgpu_genome_t *genome, int seedLen, double slack, int device);
/* Diagnostic: wall seconds of the last successful snapgpu_index_build_gpu of this process by
 * phase -- upload, scan, sort, runs, sizing, placement, write, download (8 doubles) -- and the
 * most device memory it held at once.  SNAPGPU_EINVAL when there was none. */
#define SNAPGPU_INDEX_BUILD_PHASES 8
int snapgpu_index_build_gpu_stats(double phaseSeconds[SNAPGPU_INDEX_BUILD_PHASES], uint64_t *peakDeviceBytes);
/* GenomeIndex::loadFromDirectory (GenomeIndex.cpp:844-963), reference on-disk format. */
snapgpu_index_t *snapgpu_index_load(const char *directory);
/* Write the reference on-disk format (GenomeIndex.cpp:646-710, Genome.cpp:125-158,
 * HashTable.cpp:180-215) so the reference `snap-rna` can load our index. */
int  snapgpu_index_save(const snapgpu_index_t *idx, const char *directory);
void snapgpu_index_free(snapgpu_index_t *idx);
/* Multi-rank jobs (no reference equivalent: the reference is one process): build the index
 * once per node, write it as one flat file (e.g. under /dev/shm) with snapgpu_index_share, and
 * map it read-only in every rank with snapgpu_index_attach (no private copy of the tables). */
int snapgpu_index_share(const snapgpu_index_t *idx, const char *path);
snapgpu_index_t *snapgpu_index_attach(const char *path);
/* The genome an index owns (valid while the index lives). */
const snapgpu_genome_t *snapgpu_index_genome(const snapgpu_index_t *idx);

typedef struct snapgpu_index_info {
    uint32_t nBases;
    uint32_t seedLen;
    uint32_t nHashTables;
    uint32_t chromosomePadding;
    uint64_t overflowTableSize;   /* u32 words */
    uint64_t totalHashSlots;      /* sum of tableSize */
    uint64_t totalUsedSlots;
    int32_t  nPieces;
    uint32_t hasIupac;            /* genome holds bytes other than ACGTn */
} snapgpu_index_info_t;
int snapgpu_index_get_info(const snapgpu_index_t *idx, snapgpu_index_info_t *info);

/* Raw read-only view of the index tables (SNAPHashTable entries are
 * {u32 key, u32 value1, u32 value2}, HashTable.h:117-123). */
typedef struct snapgpu_index_view {
    const uint32_t *slots;          /* all tables concatenated, 3 words per slot */
    const uint64_t *tableBase;      /* [nHashTables] slot index of table start */
    const uint64_t *tableSize;      /* [nHashTables] */
    const uint32_t *overflow;       /* overflow table (count, hits... descending) */
    const char     *genome;         /* base 0 of padded genome, [-256, nBases+256) readable */
    const uint32_t *pieceOffsets;   /* [nPieces] */
    uint32_t nBases, seedLen, nHashTables, chromosomePadding;
    int32_t  nPieces;
    uint32_t pad_;
    uint64_t overflowTableSize;
} snapgpu_index_view_t;
int snapgpu_index_get_view(const snapgpu_index_t *idx, snapgpu_index_view_t *view);

/* GenomeIndex::lookupSeed (GenomeIndex.cpp:971-1011), host side.  Writes up to
 * `cap` hits per direction; returns the true counts in nHits[2]. */
int snapgpu_index_lookup(const snapgpu_index_t *idx, const char *seedBases,
                         uint32_t nHits[2], uint32_t *hitsFwd, uint32_t *hitsRc, uint32_t cap);

/* ------------------------------------------------------------------- reads */
/* A batch of reads in host memory: read i has bases[offsets[i] .. +lengths[i])
 * and the same range of quals (Phred+33), as Read::getData/getQuality expose
 * them (Read.h:289-328).  Buffers carry >= 16 bytes of zero slack at the end. */
typedef struct snapgpu_reads {
    uint64_t  n;
    uint64_t  totalBytes;
    char     *bases;
    char     *quals;
    uint64_t *offsets;
    uint32_t *lengths;
    uint32_t *truthLocation;   /* generator ground truth (genome offset of read start), or NULL */
    uint8_t  *truthDirection;
    /* Read::clip state (Read.h:357-404), kept by snapgpu_reads_clip: the front clip and the
     * unclipped length of every read (NULL until the first clip), and the clipping applied. */
    uint32_t *frontClipped;
    uint32_t *unclippedLength;
    int32_t   clipping;        /* ReadClippingType last applied (0 = NoClipping) */
    uint32_t  nUploads;        /* device uploads of this batch; clipping is refused after the first */
    /* Read::getId (Read.h:289-328): id i = ids[idOffsets[i] .. +idLengths[i]) (FASTQ header
     * without '@'), or NULL when the batch carries no ids. */
    char     *ids;
    uint64_t *idOffsets;
    uint32_t *idLengths;
    uint32_t  hostFlags;       /* library-internal (bit 0: bases/quals in pinned host memory) */
    uint32_t  reserved_;
} snapgpu_reads_t;

/* wgsim-like simulator: uniform start, 50/50 strand,
 * haplotype mutations (rate, indel fraction) then per-base substitution errors,
 * constant quality char. */
typedef struct snapgpu_synth_reads_params {
    uint64_t seed;              /* e.g. 99 */
    uint64_t nReads;
    uint32_t readLength;        /* 100 */
    uint32_t qualityChar;       /* '2' = Q17, as wgsim writes for 2% error */
    double   baseErrorRate;     /* 0.02 */
    double   mutationRate;      /* 0.001 */
    double   indelFraction;     /* 0.15 */
    double   indelExtend;       /* 0.3 */
    double   randomReadFraction;/* fraction of reads of pure noise (NotFound) */
} snapgpu_synth_reads_params_t;
snapgpu_reads_t *snapgpu_reads_synthetic(const snapgpu_genome_t *g, const snapgpu_synth_reads_params_t *p);
/* wgsim-like read pairs (nReads pairs, readLength each): insert ~ N(insertMean, insertSd). */
int snapgpu_reads_synthetic_pairs(const snapgpu_genome_t *g, const snapgpu_synth_reads_params_t *p, uint32_t insertMean,
                                  uint32_t insertSd, snapgpu_reads_t **reads0, snapgpu_reads_t **reads1);
snapgpu_reads_t *snapgpu_reads_from_fastq(const char *path);
/* The same over nBytes of FASTQ text in memory (snapgpu_reads_from_fastq maps the file and calls
 * this).  Records are the line quadruples 4r .. 4r + 3, lines counted by '\n'; a last line without
 * a newline counts, 1-3 trailing lines are ignored.  name only appears in error messages. */
snapgpu_reads_t *snapgpu_reads_from_fastq_buffer(const char *text, uint64_t nBytes, const char *name);
/* Build a batch from caller arrays (copies them). */
snapgpu_reads_t *snapgpu_reads_from_arrays(uint64_t n, const char *bases, const char *quals,
                                           const uint64_t *offsets, const uint32_t *lengths);
int  snapgpu_reads_write_fastq(const snapgpu_reads_t *r, const char *path);
void snapgpu_reads_free(snapgpu_reads_t *r);

/* ----------------------------------------------------------------- aligner */
typedef struct snapgpu_aligner snapgpu_aligner_t;

int  snapgpu_device_count(void);
int  snapgpu_device_cu_count(int device);   /* compute units of a device (0 if none) */
/* BaseAligner::BaseAligner (BaseAligner.cpp:46-194) + index upload to HBM.  The
 * index must outlive the aligner. */
snapgpu_aligner_t *snapgpu_aligner_create(int device, const snapgpu_index_t *idx,
                                          const snapgpu_aligner_params_t *params);
void snapgpu_aligner_free(snapgpu_aligner_t *a);

/* Batched BaseAligner::AlignRead (BaseAligner.cpp:196-200 / 510-938) over host
 * buffers: H2D of the reads, the GPU passes, D2H of the records. */
int snapgpu_align_batch(snapgpu_aligner_t *a, const snapgpu_reads_t *reads, snapgpu_result_t *out);

/* Streaming form of snapgpu_align_batch for callers that keep several batches in flight (the
 * GpuSingleExtension pattern): submit returns once the batch is queued (its last chunks still
 * on the GPU; earlier batches' chunks are finished as their streams are reused); wait drains
 * everything submitted.  reads and out must stay valid, and out untouched, until the wait.
 * snapgpu_last_timing then covers every batch since the previous wait. */
int snapgpu_align_batch_submit(snapgpu_aligner_t *a, const snapgpu_reads_t *reads, snapgpu_result_t *out);
int snapgpu_align_batch_wait(snapgpu_aligner_t *a);

/* The extended AlignRead (BaseAligner.h:72-86, BaseAligner.cpp:510-938) used by the
 * paired / transcriptome callers:
 *  - per-read search window: searchRadius != 0 restricts hits to genome locations
 *    within searchRadius of searchLocation, in searchDirection only (windowed
 *    GenomeIndex::lookupSeed, GenomeIndex.cpp:1013-1086, and BaseAligner.cpp:781-853);
 *  - multi-hit export (fillHitsFound, BaseAligner.cpp:940-975, recording at :1255-1261):
 *    up to maxHitsToGet hits with edit distance in [best, best+3] per read, written to
 *    multiHits[i * maxHitsToGet ..], their count to multiHitsFound[i]; entries past
 *    multiHitsFound[i] in a read's row are left untouched (only the found hits are copied
 *    back, compacted on the device).
 * search may be NULL (no window for any read); maxHitsToGet 0 disables multi-hit
 * export (multiHitsFound / multiHits may then be NULL); at most SNAPGPU_MAX_MULTI_HITS_TO_GET.
 * The reference keeps 512 hits per distance (BaseAligner.h:148-151) but counts up to
 * maxHitsToGet per distance, so above 512 a distance's extra hits overwrite the next
 * distances' rows; that layout is reproduced (the RNA paired path asks for 1000,
 * PairedAligner.cpp:584).  maxHitsToGet > 512 needs (maxK + extraSearchDepth) * 512 +
 * maxHitsToGet <= 31 * 512 (the writes stay inside the reference's table). */
#define SNAPGPU_MAX_MULTI_HITS_TO_GET 1024
typedef struct snapgpu_search {
    uint32_t searchRadius;
    uint32_t searchLocation;
    uint32_t searchDirection;   /* SNAPGPU_FORWARD / SNAPGPU_RC */
    uint32_t reserved;
} snapgpu_search_t;
typedef struct snapgpu_multi_hit {
    uint32_t location;
    uint8_t  direction;         /* multiHitRCs */
    uint8_t  score;             /* multiHitScores */
    uint16_t reserved;
} snapgpu_multi_hit_t;
int snapgpu_align_batch_ex(snapgpu_aligner_t *a, const snapgpu_reads_t *reads, const snapgpu_search_t *search,
                           uint32_t maxHitsToGet, snapgpu_result_t *out, int32_t *multiHitsFound,
                           snapgpu_multi_hit_t *multiHits);

/* Device-resident variant: reads are uploaded once with snapgpu_reads_upload;
 * snapgpu_align_resident runs only the GPU passes (inputs already in HBM, output
 * left in HBM); snapgpu_results_download copies the records back. */
typedef struct snapgpu_device_reads snapgpu_device_reads_t;
snapgpu_device_reads_t *snapgpu_reads_upload(snapgpu_aligner_t *a, const snapgpu_reads_t *reads);
void snapgpu_device_reads_free(snapgpu_device_reads_t *d);
int  snapgpu_align_resident(snapgpu_aligner_t *a, snapgpu_device_reads_t *d);
int  snapgpu_results_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, snapgpu_result_t *out);
int  snapgpu_synchronize(snapgpu_aligner_t *a);

/* FASTQ parsed on the device (fastq_parse.hip): the text is uploaded through pinned staging and
 * split, clipped (ReadClippingType clipping, 0..3) and packed in device memory.  *dOut is what
 * snapgpu_reads_upload of the host parser's batch, clipped by snapgpu_reads_clip, would be.  With
 * SNAPGPU_FASTQ_HOST_BATCH in flags, *readsOut is that host batch itself, downloaded (free it with
 * snapgpu_reads_free); without, readsOut may be NULL and only offsets and lengths come back.
 * Synchronous.  SNAPGPU_EFORMAT, with the host parser's message, for a record without '@' header;
 * SNAPGPU_ENOMEM when the device's free memory cannot hold the call's buffers.  There is no
 * fallback to the host parser.  snapgpu_fastq_upload_file reads the file straight into the staging. */
#define SNAPGPU_FASTQ_HOST_BATCH 1u
int snapgpu_fastq_upload(snapgpu_aligner_t *a, const char *text, uint64_t nBytes, const char *name,
                         int clipping, uint32_t flags,
                         snapgpu_device_reads_t **dOut, snapgpu_reads_t **readsOut);
int snapgpu_fastq_upload_file(snapgpu_aligner_t *a, const char *path, int clipping, uint32_t flags,
                              snapgpu_device_reads_t **dOut, snapgpu_reads_t **readsOut);
/* The same over a BGZF stream of the text (bgzip's .gz; see snapgpu_bgzf_inflate_gpu below): the
 * compressed bytes are uploaded and inflated on the device straight into the parser's text buffer,
 * and the passes above run from there.  An empty stream, or only empty members (the EOF block),
 * is an empty batch.  SNAPGPU_EFORMAT for a stream that is not BGZF (plain gzip included) or has a
 * member the inflater refuses; the call frees what it allocated.  The _file form reads the
 * compressed file into host memory first. */
int snapgpu_fastq_upload_bgzf(snapgpu_aligner_t *a, const char *data, uint64_t nBytes, const char *name,
                              int clipping, uint32_t flags,
                              snapgpu_device_reads_t **dOut, snapgpu_reads_t **readsOut);
int snapgpu_fastq_upload_bgzf_file(snapgpu_aligner_t *a, const char *path, int clipping, uint32_t flags,
                                   snapgpu_device_reads_t **dOut, snapgpu_reads_t **readsOut);
/* The aligner's last snapgpu_fastq_upload*: text upload (host pass into the staging included; the
 * compressed stream's for the BGZF forms), kernels (HIP events; the inflate kernel included),
 * downloads, in ms.  SNAPGPU_EINVAL when there was none. */
int snapgpu_fastq_last_ms(snapgpu_aligner_t *a, double *uploadMs, double *kernelMs, double *downloadMs);
uint32_t snapgpu_fastq_tile_bytes(void);   /* bytes of text one workgroup scans for newlines */
/* Test accessor: a resident batch's n, bytes, longest read and extent hash; its offsets (n),
 * lengths (n), and bases and qualities (bytes + 64 each) where the pointers are not NULL. */
int snapgpu_device_reads_peek(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, uint64_t *n, uint64_t *bytes,
                              uint32_t *maxLen, uint64_t *extentHash, uint64_t *offsets, uint32_t *lengths,
                              char *bases, char *quals);
/* A batch made by snapgpu_fastq_upload* also keeps, in device memory of its own, what the SAM / BAM
 * calls below otherwise take from the host batch: the packed ids with their offsets and lengths, the
 * front clips and unclipped lengths, the bases and qualities past the largest clipped end, and the
 * longest unclipped read and longest id.  Those calls then accept reads == NULL (see
 * snapgpu_sam_resident), with or without SNAPGPU_FASTQ_HOST_BATCH.  A batch from snapgpu_reads_upload
 * keeps none of this.
 * snapgpu_device_reads_ids_download copies the ids back (waits; off the critical path of a caller
 * that formats on the device): the packed blob under the size contract of snapgpu_sam_download
 * (*used = its bytes, SNAPGPU_EINVAL if cap is too small), and, where the pointers are not NULL,
 * n entries each of idOffsets, idLengths, frontClipped and unclippedLength -- the fields of that name
 * of the host batch.  The two clip arrays are left untouched for a batch uploaded with clipping 0.
 * SNAPGPU_EINVAL for a batch without resident ids. */
int snapgpu_device_reads_ids_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, char *ids, uint64_t cap,
                                      uint64_t *used, uint64_t *idOffsets, uint32_t *idLengths,
                                      uint32_t *frontClipped, uint32_t *unclippedLength);

/* Timing of the dominant kernel (HIP events on the stream it ran on), in ms, for the last
 * snapgpu_align_resident / snapgpu_align_batch call.  snapgpu_align_batch pipelines its reads
 * in chunks over two streams: the kernel figures are then sums over its nLaunches chunks. */
typedef struct snapgpu_timing {
    double mainKernelMs;     /* the simple pass (front stream) + pass 1: align_kernel<128> (reads <= 128
                                bases, bit-plane LV) on the lane; the wait between the two is left out */
    double spillKernelMs;    /* passes 2 + 3: align_kernel<256> over the reads pass 1 deferred
                                (129..256 bases, bit-plane LV), align_kernel<512> over the rest */
    double fixupMs;          /* host MAPQ fix-ups */
    uint64_t nSpilled;       /* reads deferred by pass 1 */
    uint64_t nMapqFixed;
    double lookupKernelMs;   /* pass 0: seed_lookup_kernel (first-round seed lookups) */
    uint64_t lookupSeeds;    /* seeds it looked up */
    uint64_t lookupProbes;   /* bucket lines it loaded */
    uint64_t lookupOverflowReads; /* overflow-list counts it read */
    uint64_t nLaunches;      /* pass sets the figures above sum over (chunks of snapgpu_align_batch) */
    double wallMs;           /* snapgpu_align_batch: host reads in -> records out, whole call */
    double mainKernelBusyMs; /* union of the simple-pass and pass-1 launch intervals (the two lanes' launches
                                and the front stream's overlap) */
    double lookupKernelBusyMs;/* union of the pass-0 launch intervals */
    uint64_t nByteReads;     /* reads deferred by pass 2 to the byte-compare pass 3 (> 256 bases,
                                or IUPAC codes in both read and genome) */
    uint64_t nArenaOverflow; /* reads that outgrew a capped element arena in passes 1-3 and were
                                aligned again by the big-arena pass (worst-case arenas, small grid) */
    uint64_t nNulReads;      /* records with SNAPGPU_FLAG_NUL_BYTE (0 for any FASTQ input) */
    uint64_t nUnwritten;     /* records no pass wrote (the device output is pre-filled with 0xff
                                and every read must get exactly one record): always 0, else the
                                call fails with SNAPGPU_EDEVICE */
    uint64_t nForcedSettled; /* pass 1, forced mode: elements the lane prefilter settled (one pending
                                candidate whose distances fail), counted without being fetched */
    uint64_t nForcedLimitSpans; /* ...batches in which a success lowered the score limit ahead of such
                                elements, which were then counted with the limit at their turn */
    uint64_t nSimpleReads;   /* records written by the simple pass (simple_align_kernel: reads whose
                                seeds all point at one candidate), ahead of pass 1 */
    uint64_t nSimpleBailed;  /* reads <= 128 bases the simple pass handed on to pass 1 */
    uint64_t nSimpleWide;    /* of nSimpleReads: records written by the pass's one-read path (the reads its
                                four-reads-per-wave path hands on: a non-ACGT base, a score above 7, ...) */
} snapgpu_timing_t;
int snapgpu_last_timing(snapgpu_aligner_t *a, snapgpu_timing_t *t);

/* Aggregated getters of the reference aligner (Aligner.h:62-70). */
typedef struct snapgpu_aligner_stats {
    int64_t nHashTableLookups;
    int64_t nLocationsScored;
    int64_t nHitsIgnoredBecauseOfTooHighPopularity;
    int64_t nReadsIgnoredBecauseOfTooManyNs;
    int64_t nIndelsMerged;
    int64_t nReads;
} snapgpu_aligner_stats_t;
int snapgpu_aligner_get_stats(const snapgpu_aligner_t *a, snapgpu_aligner_stats_t *s);
int snapgpu_aligner_max_k(const snapgpu_aligner_t *a);           /* getMaxK() */
/* Whether the pass sets of the aligner's two streams may run concurrently (default 1; the
 * environment variable SNAPGPU_OVERLAP sets the initial value).  0 serialises the kernels
 * (copies and host work still overlap them): each launch's duration is then its own.  The front
 * stage of a pass set (record pre-fill, pass 0, the simple pass) runs on a third stream ahead of the
 * lanes; serialised, it waits for the previous set's last pass too. */
int snapgpu_aligner_set_overlap(snapgpu_aligner_t *a, int overlap);
/* Whether the simple pass runs ahead of pass 1 (default 1; SNAPGPU_SIMPLE_PASS sets the initial
 * value).  It never runs with stopOnFirstHit, explorePopularSeeds, maxHitsToConsider >= 0xffff, a
 * search window or multi-hit export.  Results do not depend on it. */
int snapgpu_aligner_set_simple_pass(snapgpu_aligner_t *a, int on);
/* Test hook (no reference equivalent): the aligner's next calls trip its device watchdog when
 * the batch's read `read_index` starts (0xffffffff: never), so the call fails with
 * SNAPGPU_EDEVICE.  Each aligner has its own watchdog record: a trip in one aligner neither
 * fails nor stops another aligner on the same device. */
int snapgpu_aligner_debug_trip(snapgpu_aligner_t *a, uint32_t read_index);
/* Test accessor (no reference equivalent): the persistent kernels' grids and what they were sized
 * from.  A grid is the compute units times the workgroups per CU that are resident at once: the
 * lesser of the runtime's occupancy answer and ldsPerCU / (the kernel's static LDS rounded up to
 * ldsUnit); grid256 and grid512 are capped at grid128 (they reuse its arenas).  shortRows: pass 1 runs
 * the 128-base align kernel with 16 Landau-Vishkin rows in LDS (maxK + extraSearchDepth <= 16), lds128
 * being that kernel's static LDS.  The environment variable SNAPGPU_WAVES_PER_CU caps every perCU. */
typedef struct snapgpu_grids {
    uint32_t computeUnits, shortRows;
    uint32_t perCU128, grid128;
    uint32_t perCU256, grid256;
    uint32_t perCU512, grid512;
    uint32_t perCUSimple, gridSimple;
    uint32_t perCUCigar, gridCigar;
    uint32_t lds128, ldsUnit, ldsPerCU, reserved;
    /* registers a lane of seed_lookup_kernel (pass 0) and of the 128-base align kernel is allocated
     * (hipFuncGetAttributes::numRegs rounded up to the allocation unit of 8): pass 0 runs beside the
     * resident align kernel only while 5 * vgpr128 + vgprLookup <= 512, the SIMD's register file */
    uint32_t vgprLookup, vgpr128;
} snapgpu_grids_t;
int snapgpu_aligner_debug_grids(snapgpu_aligner_t *a, snapgpu_grids_t *g);
/* SHA-256 of the sources this library was built from (snapgpu/_srcsha.py: csrc, this header, the
 * Makefile); the Python loader refuses a library whose identity differs from the sources beside it. */
const char *snapgpu_source_sha256(void);
/* Diagnostic (no reference equivalent): with SNAPGPU_PHASES=1 in the environment at
 * snapgpu_aligner_create, align_kernel<128> sums shader cycles per phase and event
 * counts into out[0..min(len, 48)) (order: snapgpu.BaseAligner.PHASES); reset != 0 zeroes them. */
int snapgpu_phase_cycles(snapgpu_aligner_t *a, uint64_t *out, uint32_t len, int reset);
const char *snapgpu_aligner_name(const snapgpu_aligner_t *a);    /* getName() */

/* -------------------------------------------------------- Landau-Vishkin */
/* LandauVishkin<dir>::computeEditDistance (LandauVishkin.h:211-455) on the GPU,
 * one call per task, for unit parity (reference tests/LandauVishkinTest.cpp).
 * Task i: text = texts[textOff[i] .. +textLen[i]) (for dir=-1 the text is
 * walked backwards from its last byte, as a reverse LV called with a pointer
 * one past the end), pattern/quals = patterns/quals[patOff[i] .. +patLen[i]).
 * Out: edit distance or -1, netIndel, matchProbability. */
int snapgpu_lv_batch(int device, int direction, uint32_t n,
                     const char *texts, const uint64_t *textOff, const uint32_t *textLen,
                     const char *patterns, const char *quals, const uint64_t *patOff,
                     const uint32_t *patLen, const int32_t *k,
                     int32_t *outScore, int32_t *outNetIndel, double *outProb);

/* Diagnostic (no reference equivalent): scoring passes as align_kernel<128> (nw = 2, reads <= 128
 * bases) and align_kernel<256> (nw = 4, reads <= 256) run them -- unit parity for the production
 * bit-plane LV (lv_pass' two lv_group calls in every lane group, then lv_prob_groups; align_score.h).
 * Pass i: the forward read reads/quals[readOff[i] .. +readLen[i]), seedLen[i], the limit k[i] (the
 * lane-group size is chosen from it as the aligner does: 64/GS = 8, 4, 2, 1 groups at k <= 3, 7,
 * 15, above) and SNAPGPU_LV_PASS_GROUPS candidate rows of 8 int64 in cand (row i * GROUPS + g is
 * lane group g; rows beyond the pass's groups must be inactive):
 *   genOff  offset in `genome` of the candidate's position 0
 *   before, after  bytes of `genome` that belong to it before position 0 / from position 0 on
 *           (positions outside never match; the reverse call reads up to MAX_K + 2 before 0, the
 *           forward one up to 2 past glen)
 *   dir     0, or 1: the reverse-complemented read, qualities reversed
 *   s       seed offset in read[dir], 0 <= s <= n - seedLen
 *   act     0: the group holds no servable candidate
 *   glen    genome bytes available (BaseAligner.cpp:1161-1185), >= s + seedLen
 *   rtl     text length of the reverse call (BaseAligner.cpp:1216-1220: s + 31)
 * Out, per row: the forward and reverse distances (-1: above the limit k / k - e1, or not reached)
 * and -- where both are >= 0 -- their match probabilities and the reverse path's netIndel. */
#define SNAPGPU_LV_PASS_GROUPS 8
int snapgpu_lv_pass_batch(int device, int nw, uint32_t nPasses, const char *reads, const char *quals,
                          uint64_t readBytes, const uint64_t *readOff, const uint32_t *readLen,
                          const int32_t *seedLen, const int32_t *k, const char *genome, uint64_t genomeBytes,
                          const int64_t *cand, int32_t *outE1, int32_t *outE2, double *outP1, double *outP2,
                          int32_t *outNetIndel);

/* Diagnostic (no reference equivalent): the forced-mode prefilter of align_kernel<128> (forced_filter,
 * align_score.h; lv_lane.h) on explicit tasks over the aligner's device genome: quad = 0 the lane-pair
 * form (limits k <= 5), quad != 0 the lane-quad form (k <= 7).  Task i: read reads[readOff[i] ..
 * +readLen[i]) (<= 128 bases), candidate location loc[i], dir[i] (1: reverse complement), seed offset
 * s[i] in read[dir], limit k[i], act[i] (0: the lanes sit the pass out).  out[i] = 0 when the task is
 * inactive or the window [loc, loc + n + 31) is not servable, else 1 << 31 | e1 << 8 | e2 << 11 with 7
 * for a distance above its limit (e2 also when the reverse call is not reached). */
int snapgpu_lv_filter_batch(snapgpu_aligner_t *a, int quad, uint32_t nTasks, const char *reads, uint64_t readBytes,
                            const uint64_t *readOff, const uint32_t *readLen, const uint32_t *loc,
                            const int32_t *dir, const int32_t *s, const int32_t *k, const int32_t *act,
                            uint32_t *out);

/* ------------------------------------------------- CIGAR / SAM records */
/* The SAM writer's per-read work, on the GPU:
 * LandauVishkinWithCigar::computeEditDistance (LandauVishkin.cpp:252-535) as
 * SAMFormat::computeCigarString (SAM.cpp:1162-1230) calls it -- text = the genome
 * substring at the location with the read's length, k = MAX_K - 1, the read
 * upper-cased and, for RC, reverse-complemented (getSAMData, SAM.cpp:866-883).
 * Per read out: editDistance (the NM tag; -1 when the reference prints "*": no
 * location, no substring (Genome::getSubstring NULL) or no alignment within k),
 * nOps, and ops[i * SNAPGPU_CIGAR_MAX_OPS ..] as BAM ops (count << 4 | code, code
 * index into "MIDNSHP=X"; useM != 0 is the `-M` form: '=' and 'X' merged into 'M').
 * snapgpu_cigar_batch writes the first nOps[i] entries of row i only.
 * Reads longer than 512 bases are rejected (SNAPGPU_EINVAL). */
#define SNAPGPU_CIGAR_MAX_OPS 64

/* Explicit (location, direction) per read; location 0xffffffff => "*". */
int snapgpu_cigar_batch(snapgpu_aligner_t *a, const snapgpu_reads_t *reads, const uint32_t *locations,
                        const uint8_t *directions, int useM, int32_t *editDistance, uint32_t *nOps, uint32_t *ops);
/* Device-resident: the CIGARs of the records the last snapgpu_align_resident left
 * in HBM for these reads, with writeRead's rules (SAM.cpp:1007-1048, 855-883): a
 * NotFound record keeps its location for the CIGAR but uses the forward read. */
int snapgpu_cigar_resident(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, int useM);
int snapgpu_cigar_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, int32_t *editDistance, uint32_t *nOps,
                           uint32_t *ops);
/* cigar_kernel time of the last snapgpu_cigar_resident / snapgpu_cigar_batch (HIP events). */
int snapgpu_cigar_last_ms(snapgpu_aligner_t *a, double *ms);

/* One SAM line per read, as SAMFormat::writeRead (SAM.cpp:1007-1155) writes it for a
 * single-end genome alignment: QNAME (read id up to the first space), FLAG, RNAME,
 * POS, MAPQ (clamped to [0, 70]; 0 when unmapped), CIGAR, "*", 0, 0, SEQ and QUAL
 * (reverse-complemented / reversed for RC), RG:Z:<readGroup> (omitted when NULL),
 * PG:Z:SNAP, NM:i:<editDistance>.  ids[idOffsets[i] .. +idLengths[i]) is read i's
 * id.  Writes at most `cap` bytes to out and the size needed to *used; returns
 * SNAPGPU_EINVAL (nothing usable written) when cap is too small. */
int snapgpu_sam_format(const snapgpu_index_t *idx, const snapgpu_reads_t *reads, const char *ids,
                       const uint64_t *idOffsets, const uint32_t *idLengths, const snapgpu_result_t *results,
                       const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                       const char *readGroup, char *out, uint64_t cap, uint64_t *used);

/* Clipped reads (Read::clip, Read.h:357-404, applied by the FASTQ reader, FASTQ.cpp:250;
 * clipping = NoClipping 0 / ClipFront 1 / ClipBack 2 / ClipFrontAndBack 3 -- the reference's
 * default is 3): snapgpu_reads_clip narrows offsets/lengths in place to the clipped read (what
 * the aligner and the CIGAR kernel see) and returns the front clip and unclipped length per
 * read; snapgpu_sam_format_clipped then prints the unclipped SEQ/QUAL and the soft clips
 * ("%uS" before / after the CIGAR, mirrored for RC -- SAM.cpp:866-883, 1212-1226). */
int snapgpu_reads_clip(snapgpu_reads_t *reads, int clipping, uint32_t *frontClipped, uint32_t *unclippedLength);
int snapgpu_sam_format_clipped(const snapgpu_index_t *idx, const snapgpu_reads_t *reads, const char *ids,
                               const uint64_t *idOffsets, const uint32_t *idLengths, const snapgpu_result_t *results,
                               const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                               const char *readGroup, const uint32_t *frontClipped, const uint32_t *unclippedLength,
                               char *out, uint64_t cap, uint64_t *used);

/* The same lines written on the GPU (sam_format.hip: a length pass, an exclusive scan into 64-bit
 * line starts and a write pass that stages each workgroup's byte range in LDS), so that only the
 * text crosses PCIe.  Byte-identical to snapgpu_sam_format / snapgpu_sam_format_clipped; the host
 * formatter stays the default of the product paths.  There is no fallback to it: a failure is an
 * error.  After the write pass a device check counts the lines whose last byte is not '\n' where
 * the scan placed it: always 0, else the download fails with SNAPGPU_EDEVICE. */
/* Resident: SAM lines of the records and CIGARs that snapgpu_align_resident + snapgpu_cigar_resident
 * left in HBM for d.  reads is the batch d was uploaded from (n and lengths are checked); its clip
 * state is used.  ids/idOffsets/idLengths NULL => reads->ids...; asynchronous on the side stream
 * (the next snapgpu_align_resident waits for it before it rewrites the records).  SNAPGPU_EINVAL:
 * no snapgpu_cigar_resident before, a reads batch that does not match d, an unclipped read longer
 * than 1024 bases, no ids at all.
 * reads == NULL: the batch's own resident ids and clip state, which only snapgpu_fastq_upload* leaves
 * (SNAPGPU_EINVAL for a batch from snapgpu_reads_upload).  Nothing per read is then uploaded: the
 * kernels read the ids, clip arrays and unclipped bases / qualities the parser left in device memory,
 * the text bound comes from the batch's totals, and the 1024-base limit is checked against the
 * longest unclipped read found at upload time.  There is no extent check (nothing to compare).  The
 * text is byte-identical to the call with the host batch.  Caller ids (ids, idOffsets and idLengths
 * all non-NULL) are still taken, and uploaded, with reads == NULL.  Calls with and without reads may
 * alternate on one batch.  The same holds for snapgpu_sam_resident_sorted and snapgpu_bam_resident /
 * _sorted (whose 254-byte id limit is checked against the longest id found at upload time). */
int snapgpu_sam_resident(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, const snapgpu_reads_t *reads,
                         const char *ids, const uint64_t *idOffsets, const uint32_t *idLengths,
                         const char *readGroup);
/* Waits; same size contract as snapgpu_sam_format: *used = bytes needed, SNAPGPU_EINVAL if cap is
 * too small (nothing usable written). */
int snapgpu_sam_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, char *out, uint64_t cap, uint64_t *used);
/* Batch form, for callers and tests that hold records and CIGARs on the host: the arguments of
 * snapgpu_sam_format_clipped with the aligner in place of the index; uploads, runs the same
 * kernels, downloads. */
int snapgpu_sam_format_gpu(snapgpu_aligner_t *a, const snapgpu_reads_t *reads, const char *ids,
                           const uint64_t *idOffsets, const uint32_t *idLengths, const snapgpu_result_t *results,
                           const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                           const char *readGroup, const uint32_t *frontClipped, const uint32_t *unclippedLength,
                           char *out, uint64_t cap, uint64_t *used);
/* kernel time (length + scan + write, HIP events; a sorted call's sort step included) and download
 * time of the last call */
int snapgpu_sam_last_ms(snapgpu_aligner_t *a, double *kernelMs, double *downloadMs);
/* Diagnostic: the kernel time of the last call by pass -- length, scan, write (with the check).  A
 * sorted call's sort step is in none of the three (snapgpu_sam_sort_ms). */
int snapgpu_sam_pass_ms(snapgpu_aligner_t *a, double *lengthMs, double *scanMs, double *writeMs);

/* `-so` on the device: the same lines in coordinate order (@HD SO:coordinate, snapgpu_sam_header with
 * sorted = 1).  The sort key is SAMFormat::getSortInfo's location (SAM.cpp:639-685) of the line,
 * computed from the record by the length pass, not parsed from text: 0xffffffff when RNAME is "*"
 * or the piece's name is empty or begins with '*', else the offset of the first piece of that name
 * + POS - 1.  A stable radix sort of (key, record index) follows the length pass; the scan and the
 * write pass then run over output slots.  One call is one sort block, as in the product paths.
 * Contract: the text is byte-identical to snapgpu_sam_sort_records(idx, <the unsorted text of the
 * same call>) whenever no QNAME (the id up to its first space) holds a tab or a line feed.  With
 * such a byte in a QNAME the host sorter reads shifted fields; the device order still follows the
 * record's own key and is the one to trust.  There is no refusal and no scan of the ids. */
/* snapgpu_sam_resident in coordinate order: same arguments, checks, asynchrony and ordering against
 * the next snapgpu_align_resident; snapgpu_sam_download then returns the sorted text. */
int snapgpu_sam_resident_sorted(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, const snapgpu_reads_t *reads,
                                const char *ids, const uint64_t *idOffsets, const uint32_t *idLengths,
                                const char *readGroup);
/* Waits; order[j] = the record (read index) whose line is the j-th of the sorted text, n entries: a
 * caller reorders whatever else it keeps per read by it.  SNAPGPU_EINVAL when the batch's last SAM
 * call was not snapgpu_sam_resident_sorted, or there was none. */
int snapgpu_sam_order_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, uint32_t *order);
/* The batch form of the sorted call: snapgpu_sam_format_gpu's arguments, then order (n entries as
 * above, or NULL). */
int snapgpu_sam_format_gpu_sorted(snapgpu_aligner_t *a, const snapgpu_reads_t *reads, const char *ids,
                                  const uint64_t *idOffsets, const uint32_t *idLengths, const snapgpu_result_t *results,
                                  const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                                  const char *readGroup, const uint32_t *frontClipped, const uint32_t *unclippedLength,
                                  char *out, uint64_t cap, uint64_t *used, uint32_t *order);
/* The sort keys above of n records, computed on the host by the code the device length pass runs.
 * Needs no GPU.  A stable argsort of them is the order of the sorted calls. */
int snapgpu_sam_sort_keys(const snapgpu_index_t *idx, uint64_t n, const snapgpu_result_t *results, uint32_t *keys);
/* HIP-event time of the sort step of the last device SAM call (order fill, radix sort, gather of the
 * lengths); 0 after an unsorted call. */
int snapgpu_sam_sort_ms(snapgpu_aligner_t *a, double *sortMs);
/* The exact byte length of every line snapgpu_sam_format_clipped prints (same arguments, same
 * validation; NULL clip arrays mean the batch's own clip state, or unclipped), computed on the host
 * by the code the device length pass runs.  Needs no GPU. */
int snapgpu_sam_line_lengths(const snapgpu_index_t *idx, const snapgpu_reads_t *reads, const char *ids,
                             const uint64_t *idOffsets, const uint32_t *idLengths, const snapgpu_result_t *results,
                             const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                             const char *readGroup, const uint32_t *frontClipped, const uint32_t *unclippedLength,
                             uint32_t *lineLengths);

/* The SAM header as SAMFormat::writeHeader (SAM.cpp:700-800) writes it for a FASTQ input:
 * @HD (SO:coordinate if sorted), rgLine or "@RG\tID:FASTQ\tSM:sample", @PG with CL:commandLine
 * and VN:version, one @SQ per genome piece.  Same size / error contract as snapgpu_sam_format. */
int snapgpu_sam_header(const snapgpu_index_t *idx, int sorted, const char *commandLine, const char *version,
                       const char *rgLine, char *out, uint64_t cap, uint64_t *used);

/* ------------------------------------------------------------ BAM records (reads without mate)
 * One uncompressed BAM record per read, as BAMFormat::writeRead (Bam.cpp:596-790) writes it for a
 * single-end genome alignment, appended in input order: the arguments of snapgpu_sam_format_clipped
 * (NULL clip arrays: the batch's own clip state, or unclipped), the same limits (unclipped read <=
 * 1024 bases, nOps <= SNAPGPU_CIGAR_MAX_OPS) and the same size contract as snapgpu_sam_format.
 * Unlike the SAM line: QNAME is the whole id (not cut at the first space; a batch with an id longer
 * than 254 bytes is refused with SNAPGPU_EINVAL -- the reference exits, Bam.cpp:723-726); SEQ and
 * QUAL cover the whole unclipped read; the record's location decides CIGAR ops, bin and NM even for
 * a NotFound record, while refID, pos, FLAG and MAPQ take NotFound as unmapped.
 * NM carry (writeRead's editDistance is only assigned when it computes a CIGAR, Bam.cpp:644,
 * 654-679, 780): nm[i] = editDistance[i] when record i gets CIGAR ops (location valid and
 * editDistance[i] >= 0), else nm[i - 1], with nm[-1] = nmCarryIn; *nmCarryOut (may be NULL) = nm[n - 1],
 * or nmCarryIn for n == 0 -- pass it to the next batch of the same output.
 * Known gap: where LV fails at a valid genome substring the reference writes NM -1; editDistance -1
 * does not tell that case from a read off the contig's end, so the rule above carries the previous
 * value there as well. */
int snapgpu_bam_format(const snapgpu_index_t *idx, const snapgpu_reads_t *reads, const char *ids,
                       const uint64_t *idOffsets, const uint32_t *idLengths, const snapgpu_result_t *results,
                       const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops, const char *readGroup,
                       const uint32_t *frontClipped, const uint32_t *unclippedLength, int32_t nmCarryIn,
                       int32_t *nmCarryOut, char *out, uint64_t cap, uint64_t *used);
/* The exact byte size of every record above (block_size + 4): same inputs, same validation. */
int snapgpu_bam_record_lengths(const snapgpu_index_t *idx, const snapgpu_reads_t *reads, const char *ids,
                               const uint64_t *idOffsets, const uint32_t *idLengths, const snapgpu_result_t *results,
                               const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                               const char *readGroup, const uint32_t *frontClipped, const uint32_t *unclippedLength,
                               uint32_t *recordLengths);
/* BAMFormat::getSortInfo (Bam.cpp:474-495) for a read without mate: the record's genome location
 * (the offset of piece refID + pos) when it has a refID, else 0xffffffff.  Unlike the SAM key
 * (snapgpu_sam_sort_keys) it goes by piece index, not by the first piece of that name: the two differ
 * where two pieces share a name, or a name is empty or begins with '*'. */
int snapgpu_bam_sort_keys(const snapgpu_index_t *idx, uint64_t n, const snapgpu_result_t *results, uint32_t *keys);
/* BAMFormat::writeHeader (Bam.cpp:542-594): magic, the n bytes of SAM header text, one reference
 * entry per genome piece (l_ref = piece span - 500).  Size contract as snapgpu_sam_header. */
int snapgpu_bam_header(const snapgpu_index_t *idx, const char *samHeaderText, uint64_t n, char *out, uint64_t cap,
                       uint64_t *used);
/* BGZF, as the product paths' ".bam" output writes it: blocks of 0xff00 input bytes, each its own
 * deflate stream in a gzip member with the BC extra field, then (eof != 0) the 28-byte EOF block.
 * The blocks are compressed on the host thread pool; the bytes are the same for every thread count.
 * Size contract as snapgpu_sam_format (n + n / 0xff00 * 128 + 256 bytes always suffice). */
int snapgpu_bgzf_compress(const char *in, uint64_t n, int eof, char *out, uint64_t cap, uint64_t *used);

/* The same records written on the GPU (bam_format.hip): a length pass (record sizes, each record's own
 * NM or none, the sort key for sorted calls), a "last defined value" scan of the NM values over
 * input order seeded with nmCarryIn, an exclusive scan of the sizes into 64-bit record starts, and a
 * write pass that stages each workgroup's byte range in LDS.  Byte-identical to snapgpu_bam_format.
 * There is no fallback to it: a failure is an error.  After the write pass a device check counts the
 * records whose block_size is not what the scan gave them: always 0, else the download fails with
 * SNAPGPU_EDEVICE.
 * snapgpu_bam_resident: arguments, checks, asynchrony and ordering against the next
 * snapgpu_align_resident as snapgpu_sam_resident; also SNAPGPU_EINVAL for an id longer than 254 bytes.
 * The BAM state of a resident batch is its own: SAM and BAM calls on one batch do not disturb each other.
 * _sorted: the records in the stable order of snapgpu_bam_sort_keys.  The NM carry still runs over
 * input order (the reference's writer runs before its sort filter). */
int snapgpu_bam_resident(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, const snapgpu_reads_t *reads,
                         const char *ids, const uint64_t *idOffsets, const uint32_t *idLengths,
                         const char *readGroup, int32_t nmCarryIn);
int snapgpu_bam_resident_sorted(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, const snapgpu_reads_t *reads,
                                const char *ids, const uint64_t *idOffsets, const uint32_t *idLengths,
                                const char *readGroup, int32_t nmCarryIn);
/* Waits; size contract as snapgpu_sam_download.  *nmCarryOut (may be NULL) = the NM of the last
 * record in input order (nmCarryIn for an empty batch). */
int snapgpu_bam_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, char *out, uint64_t cap, uint64_t *used,
                         int32_t *nmCarryOut);
/* Waits; order[j] = the read whose record is the j-th of the sorted output.  SNAPGPU_EINVAL when the
 * batch's last BAM call was not snapgpu_bam_resident_sorted, or there was none. */
int snapgpu_bam_order_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, uint32_t *order);
/* Batch form: the arguments of snapgpu_bam_format with the aligner in place of the index, then
 * sorted (0 / 1) and order (n entries written by a sorted call, or NULL). */
int snapgpu_bam_format_gpu(snapgpu_aligner_t *a, const snapgpu_reads_t *reads, const char *ids,
                           const uint64_t *idOffsets, const uint32_t *idLengths, const snapgpu_result_t *results,
                           const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                           const char *readGroup, const uint32_t *frontClipped, const uint32_t *unclippedLength,
                           int32_t nmCarryIn, int32_t *nmCarryOut, char *out, uint64_t cap, uint64_t *used, int sorted,
                           uint32_t *order);
/* kernel time (HIP events over all passes) and download time of the last device BAM call */
int snapgpu_bam_last_ms(snapgpu_aligner_t *a, double *kernelMs, double *downloadMs);

/* BGZF on the GPU (bgzf.hip over bgzf_block.h): the same split into blocks of 0xff00 input bytes and
 * the same member format as snapgpu_bgzf_compress, each member's deflate stream written by one
 * workgroup: LZ77 matches (length 4 .. 258, distance 1 .. 32768, inside the block) in one
 * dynamic-Huffman block, or a stored block where that is smaller, so a member is at most m + 31 bytes.
 * A compress pass writes every member into its own slot, a scan places them and a gather pass packs
 * them, so only the compressed bytes cross to the host.  The stream is a pure function of the input
 * (bgzf_block.h); it is not the stream zlib writes.  There is no fallback to zlib: a failure is an
 * error.  A device check counts the members that do not carry the size the scan gave them: always 0,
 * else the download fails with SNAPGPU_EDEVICE.
 * snapgpu_bam_bgzf_resident: asynchronous, on the stream of the BAM passes; compresses the records of
 * the batch's last snapgpu_bam_resident / _sorted call, in that call's order (SNAPGPU_EINVAL when
 * there was none).  A later snapgpu_bam_resident* on the batch invalidates the compressed stream.
 * snapgpu_bam_bgzf_download: waits; size contract as snapgpu_bam_download; eof != 0 appends the
 * 28-byte EOF block.  SNAPGPU_EINVAL without a snapgpu_bam_bgzf_resident since the batch's last
 * snapgpu_bam_resident*.  snapgpu_bam_download of the batch still returns the records afterwards.
 * snapgpu_bgzf_compress_gpu: the batch form for any n bytes (upload, the same kernels, download).
 * snapgpu_bgzf_compress_model: the same stream from the host thread pool, byte for byte, for every
 * input and thread count; needs no GPU.
 * snapgpu_bgzf_last_ms: kernel time (HIP events over all passes) and download time of the aligner's
 * last device BGZF call. */
int snapgpu_bam_bgzf_resident(snapgpu_aligner_t *a, snapgpu_device_reads_t *d);
int snapgpu_bam_bgzf_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, int eof, char *out, uint64_t cap,
                              uint64_t *used);
int snapgpu_bgzf_compress_gpu(snapgpu_aligner_t *a, const char *in, uint64_t n, int eof, char *out, uint64_t cap,
                              uint64_t *used);
int snapgpu_bgzf_compress_model(const char *in, uint64_t n, int eof, char *out, uint64_t cap, uint64_t *used);
int snapgpu_bgzf_last_ms(snapgpu_aligner_t *a, double *kernelMs, double *downloadMs);

/* The .bai index (SAMv1 5.2) of a coordinate-sorted record stream and a BGZF stream of it, in one
 * canonical form (csrc/bai_index.h): per reference the records' own bins ascending, a
 * bin's chunks the maximal runs of consecutive records that carry it, pseudo-bin 37450, the linear
 * index back-filled as htslib does, then n_no_coor.  streamOffset: the compressed bytes that precede
 * the record stream in the file (the BGZF of the BAM header), < 2^48.
 * snapgpu_bai_build: the host model; bgzf is any BGZF stream of the n bytes at records (an EOF block
 * may end it).  SNAPGPU_EFORMAT naming the record's index for a truncated record, refID outside
 * [-1, nRef), pos < 0 with a refID, an end past 2^29 or records out of (refID, pos) order (-1 last);
 * SNAPGPU_EINVAL when the members' ISIZEs do not sum to n.  Size contract as snapgpu_sam_format.
 * snapgpu_bai_size_bound: what an index of nRecords records over nRef references can take at most.
 * snapgpu_bam_bai_resident: asynchronous, on the stream of the BAM and BGZF passes (bai.hip): the
 * index of the batch's last snapgpu_bam_resident_sorted records over the members of the
 * snapgpu_bam_bgzf_resident that followed it (SNAPGPU_EINVAL when the last BAM call was not the sorted
 * one, when no BGZF call followed it, when streamOffset >= 2^48); nRef is the genome's contig count.
 * A later snapgpu_bam_resident* or snapgpu_bam_bgzf_resident makes it stale.
 * snapgpu_bam_bai_download: waits; *used = the index's bytes, SNAPGPU_EINVAL if cap is too small or
 * the index is stale; SNAPGPU_EDEVICE if the device counted a refused or unsorted record.
 * snapgpu_bai_build_gpu: the batch form over n bytes of records: upload, device BGZF (no EOF block),
 * index, both downloads.  A truncated record is SNAPGPU_EFORMAT; whatever else snapgpu_bai_build
 * refuses is SNAPGPU_EDEVICE here.
 * snapgpu_bai_last_ms: kernel time (HIP events over all passes) and download time of the aligner's
 * last device index. */
uint64_t snapgpu_bai_size_bound(uint64_t nRecords, uint64_t nRef, uint64_t recordBytes);
int snapgpu_bai_build(const char *records, uint64_t n, int32_t nRef, const char *bgzf, uint64_t bgzfBytes,
                      uint64_t streamOffset, char *out, uint64_t cap, uint64_t *used);
int snapgpu_bam_bai_resident(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, uint64_t streamOffset);
int snapgpu_bam_bai_download(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, char *out, uint64_t cap, uint64_t *used);
int snapgpu_bai_build_gpu(snapgpu_aligner_t *a, const char *records, uint64_t n, int32_t nRef, uint64_t streamOffset,
                          char *bgzfOut, uint64_t bgzfCap, uint64_t *bgzfUsed, char *baiOut, uint64_t baiCap,
                          uint64_t *baiUsed);
int snapgpu_bai_last_ms(snapgpu_aligner_t *a, double *kernelMs, double *downloadMs);

/* Duplicate marking (FLAG 0x400) over a coordinate-sorted stream of single-end BAM records, in one
 * canonical form (csrc/dupmark_rule.h): a record is considered when it has a refID, pos >= 0
 * and FLAG 0x4 clear; the considered records of one (refID, pos, FLAG & 0x10) are a group; a record's
 * score is the sum of its QUAL bytes, 0xff counting 0; the group's highest score is kept, the earliest
 * of the stream among equals; every other record of the group gets 0x400 and every record that is not
 * marked has it cleared.  Only byte 19 of a record ever changes, and a second application changes nothing.
 * snapgpu_bam_mark_duplicates: the host model, in place over the n bytes at records; *nGroups counts the
 * groups of two or more.  SNAPGPU_EFORMAT naming the record's index for what snapgpu_bai_build refuses
 * (a truncated record, refID outside [-1, nRef), pos < 0 with a refID, an end past 2^29, records out of
 * order), for l_seq > 2^24 and for QUAL passing the record's end; SNAPGPU_EINVAL for a record with a
 * mate (FLAG 0x1: the mate rule is not built).  A refused stream is left as it was.
 * snapgpu_bam_dupmark_resident: asynchronous, on the stream of the BAM passes (dupmark.hip): marks the
 * records of the batch's last snapgpu_bam_resident_sorted where they lie (SNAPGPU_EINVAL when the last
 * BAM call was not the sorted one).  The batch's compressed stream and index become stale, as after a
 * new snapgpu_bam_resident*; snapgpu_bam_download then returns the marked records (SNAPGPU_EDEVICE if
 * the device counted a refused or mate-carrying record, or marks that do not add up to the groups'
 * sizes).  A later snapgpu_bam_resident* writes the records again, unmarked.
 * snapgpu_bam_dupmark_stats: waits; the marked records and the groups of two or more; SNAPGPU_EINVAL
 * without a mark call since the batch's last BAM call, SNAPGPU_EDEVICE as snapgpu_bam_download.
 * snapgpu_bam_mark_duplicates_gpu: the batch form: upload, the same kernels, download in place.  A
 * truncated record is SNAPGPU_EFORMAT; whatever else the model refuses is SNAPGPU_EDEVICE here, and
 * the caller's records stay as they were.
 * snapgpu_bam_dupmark_last_ms: kernel time (HIP events over all passes) and, for the batch form, the
 * download time of the aligner's last device marking. */
int snapgpu_bam_mark_duplicates(char *records, uint64_t n, int32_t nRef, uint64_t *nMarked, uint64_t *nGroups);
int snapgpu_bam_dupmark_resident(snapgpu_aligner_t *a, snapgpu_device_reads_t *d);
int snapgpu_bam_dupmark_stats(snapgpu_aligner_t *a, snapgpu_device_reads_t *d, uint64_t *nMarked, uint64_t *nGroups);
int snapgpu_bam_mark_duplicates_gpu(snapgpu_aligner_t *a, char *records, uint64_t n, int32_t nRef, uint64_t *nMarked,
                                    uint64_t *nGroups);
int snapgpu_bam_dupmark_last_ms(snapgpu_aligner_t *a, double *kernelMs, double *downloadMs);

/* BGZF inflated (host/inflate.cpp, inflate.hip over inflate_block.h): a stream of BGZF members, as
 * bgzip, samtools and the compressors above write them, back to its bytes.  Every form first walks
 * the members (magic, CM 8, FLG 4, a BC subfield anywhere in the extra field, BSIZE inside the
 * stream, ISIZE <= 65,536, nothing after the last member); what fails there, a plain gzip file
 * included, is SNAPGPU_EFORMAT with the member's index and byte offset.  A member is accepted
 * exactly when zlib's raw inflater accepts its deflate stream with ISIZE bytes out and the trailer's
 * CRC32; otherwise SNAPGPU_EFORMAT names the lowest refused member (and, for the model and the
 * device, the status of inflate_block.h).  Size contract as snapgpu_bgzf_compress*: *used = bytes
 * needed, SNAPGPU_EINVAL when cap is too small.
 * snapgpu_bgzf_inflate_size: the walk alone.
 * snapgpu_bgzf_inflate: zlib, members spread over the host threads.
 * snapgpu_bgzf_inflate_model: inflate_block.h on the host threads, the code the kernel compiles;
 * needs no GPU and no zlib.
 * snapgpu_bgzf_inflate_gpu: upload, one wave per member, download.  No fallback to the host;
 * SNAPGPU_ENOMEM when the device's free memory cannot hold the stream and its output.
 * snapgpu_bgzf_inflate_last_ms: upload (staging pass included), kernel (HIP events) and download of
 * the aligner's last device inflate, the one inside snapgpu_fastq_upload_bgzf* included.
 * snapgpu_bgzf_inflate_waves: waves the inflate kernel launches on this aligner's device (> 0). */
int snapgpu_bgzf_inflate_size(const char *in, uint64_t n, uint64_t *outBytes, uint64_t *nMembers);
int snapgpu_bgzf_inflate(const char *in, uint64_t n, char *out, uint64_t cap, uint64_t *used);
int snapgpu_bgzf_inflate_model(const char *in, uint64_t n, char *out, uint64_t cap, uint64_t *used);
int snapgpu_bgzf_inflate_gpu(snapgpu_aligner_t *a, const char *in, uint64_t n, char *out, uint64_t cap, uint64_t *used);
int snapgpu_bgzf_inflate_last_ms(snapgpu_aligner_t *a, double *uploadMs, double *kernelMs, double *downloadMs);
int snapgpu_bgzf_inflate_waves(snapgpu_aligner_t *a);

/* --------------------------------------------- RNA annotation (GTF) */
/* GTFReader (SNAPLib/GTFReader.cpp): exon lines of a GTF/GFF3 file -> transcripts, each an
 * exon list sorted by start with an intron feature between consecutive exons (Load :1245,
 * Parse :1302, GTFTranscript::Process :972). */
typedef struct snapgpu_gtf snapgpu_gtf_t;
snapgpu_gtf_t *snapgpu_gtf_load(const char *path);
void snapgpu_gtf_free(snapgpu_gtf_t *gtf);
int snapgpu_gtf_counts(const snapgpu_gtf_t *gtf, uint32_t *nFeatures, uint32_t *nTranscripts, uint32_t *nGenes);
/* GTFReader::BuildTranscriptome (GTFReader.cpp:1840-1867): the FASTA `snap-rna transcriptome`
 * indexes -- every transcript (id order) as the genome bytes of its exon/intron list. */
int snapgpu_gtf_write_transcriptome(const snapgpu_gtf_t *gtf, const snapgpu_genome_t *genome, const char *fastaPath);
/* GTFTranscript::GenomicPosition (GTFReader.cpp:1075-1105): 1-based transcript position ->
 * 1-based genomic position (0 when the span runs past the transcript). */
int snapgpu_gtf_genomic_position(const snapgpu_gtf_t *gtf, const char *transcriptId, uint32_t pos, uint32_t span,
                                 uint32_t *genomicPos);
/* LandauVishkinWithCigar::insertSpliceJunctions (LandauVishkin.cpp:119-250): the CIGAR of a
 * transcriptome alignment at 1-based transcript position `pos`, given as (count, op) tokens,
 * with 'N' runs inserted at the transcript's junctions.  NUL-terminated string out. */
int snapgpu_gtf_splice_cigar(const snapgpu_gtf_t *gtf, const char *transcriptId, uint32_t pos, uint32_t nTokens,
                             const uint32_t *counts, const char *ops, char *out, uint64_t cap, uint64_t *used);

/* ----------------------------------- single-end product path (f1) */
/* SingleAlignerContext::runIterationThread (SNAPLib/SingleAligner.cpp:141-320) batched on the
 * GPU: per read Read::clip, the quality / length / N pre-filter (:247-257), the transcriptome
 * and genome BaseAligner::AlignRead (two aligners, :270-276), AlignmentFilter::AddAlignment /
 * FilterSingle (AlignmentFilter.cpp:140-300) and SAMFormat::writeRead (SAM.cpp:978-1153:
 * GPU CIGARs, transcriptome records with insertSpliceJunctions) -- the SAM file `snap-rna single
 * <genome> <transcriptome> <gtf> <reads>` writes, and the gene read counts FilterSingle records
 * (snapgpu_gtf_write_counts writes the count files).  Not built: the contamination database (-x),
 * BAM / sorted output. */
typedef struct snapgpu_single_options {
    int32_t  clipping;               /* ReadClippingType, default 3 = ClipFrontAndBack (AlignerOptions.cpp:48) */
    uint32_t confDiff;               /* -c, default 2 */
    uint32_t maxDist;                /* -d, default 14 (the filter's maxDist) */
    float    minPercentAbovePhred;   /* -fp, default 90 */
    uint32_t minPhred;               /* -fm, default 20 */
    uint32_t phredOffset;            /* -fo, default 33 */
    uint32_t useM;                   /* -M */
    uint32_t sortOutput;             /* -so: SAM records stable-sorted by location, @HD SO:coordinate
                                        (SortedDataWriter.cpp:186-240; one block per call; not for BAM) */
    const char *readGroup;           /* default "FASTQ" (AlignerOptions.cpp:65) */
    const char *commandLine;         /* @PG CL: */
    const char *version;             /* @PG VN: */
    /* -ct: the contamination database (SingleAligner.cpp:205-218, 282-293): reads the filter left
     * NotFound go through this BaseAligner (same parameters as the genome aligner) and each one it
     * aligns is counted in `contaminants` (both NULL: no contamination database) */
    struct snapgpu_aligner *contaminationAligner;
    struct snapgpu_contaminants *contaminants;
} snapgpu_single_options_t;
void snapgpu_single_options_default(snapgpu_single_options_t *o);

typedef struct snapgpu_single_stats {   /* AlignerStats (AlignerStats.h:40-69) */
    uint64_t totalReads, usefulReads, singleHits, multiHits, notFound, transcriptomeRecords;
    double alignMs, cigarMs, filterMs, writeMs, wallMs;
    double prepMs;   /* clipping, pre-filter, the batch view and the per-read arrays (before alignMs) */
    double formatMs, ioMs;   /* of writeMs: the records' text (host threads), the file output */
} snapgpu_single_stats_t;

/* reads: a FASTQ batch with ids (snapgpu_reads_from_fastq), clipped here.  samPath receives
 * the header and one record per read in input order: SAM text, or BGZF-compressed BAM when the
 * path ends in ".bam" (BAMFormat::writeHeader / writeRead, Bam.cpp:542-790). */
int snapgpu_single_align(snapgpu_aligner_t *genomeAligner, snapgpu_aligner_t *transcriptomeAligner,
                         snapgpu_gtf_t *gtf, snapgpu_reads_t *reads, const snapgpu_single_options_t *opt,
                         const char *samPath, snapgpu_single_stats_t *stats);
/* `-so` for SAM text (SortedDataFilter::onNextBatch, SortedDataWriter.cpp:186-240): the records
 * (lines) of `in` stable-sorted by SAMFormat::getSortInfo's location (SAM.cpp:639-685) over idx's
 * genome; header lines (starting '@') are not records and must not be in `in`.  Writes at most cap
 * bytes to out, *used = the size (= n); the product paths use it with sortOutput set. */
int snapgpu_sam_sort_records(const snapgpu_index_t *idx, const char *in, uint64_t n, char *out, uint64_t cap,
                             uint64_t *used);

/* ------------------------------------------ contamination database (-ct) counts */
/* ContaminationFilter (ContaminationFilter.cpp:22-112): contaminant alignments counted per contig
 * of the contamination genome (a location maps to its piece, Genome::getPieceAtLocation; an
 * invalid location counts nothing).  Counts accumulate over the product-path calls that carry the
 * object in their options; thread-safe. */
typedef struct snapgpu_contaminants snapgpu_contaminants_t;
snapgpu_contaminants_t *snapgpu_contaminants_create(const snapgpu_index_t *contamination);
void snapgpu_contaminants_free(snapgpu_contaminants_t *c);
int snapgpu_contaminants_add(snapgpu_contaminants_t *c, uint32_t location);   /* AddAlignment */
/* ContaminationFilter::Write: "<prefix>.contaminants.txt" with prefix = outputFileTemplate up to
 * its last '.' ("default" for NULL), one "contig<TAB>count" line per contig, by count descending
 * (the reference's std::sort over the name-ordered counts, reverse iterators) */
int snapgpu_contaminants_write(const snapgpu_contaminants_t *c, const char *outputFileTemplate);
/* the same text into out (at most cap bytes; *used = the size needed) */
int snapgpu_contaminants_format(const snapgpu_contaminants_t *c, char *out, uint64_t cap, uint64_t *used);

/* The index an aligner was created over (BaseAligner's GenomeIndex; getGenome for the SAM writer). */
const snapgpu_index_t *snapgpu_aligner_index(const snapgpu_aligner_t *a);
int snapgpu_aligner_get_params(const snapgpu_aligner_t *a, snapgpu_aligner_params_t *p);

/* Roofline calibration (diagnostic, no reference equivalent): time of nLoads independent
 * 64-byte bucket-line loads at hashed positions of this aligner's resident bucket image
 * (the access pattern of the seed lookups without their dependency chain), best of 3, ms. */
int snapgpu_gather_peak(snapgpu_aligner_t *a, uint32_t nLoads, double *ms);

/* The device image of the seed tables (no reference equivalent: SNAPHashTable's key -> value map
 * re-laid into 64-byte buckets of four {key, value1, value2, counts} entries when the aligner is
 * created; GenomeIndex::lookupSeed answers are unchanged).  Diagnostic figures of that image. */
typedef struct snapgpu_bucket_info {
    uint64_t nSlots;            /* reference-format slots the image was built from */
    uint64_t nKeys;             /* keys it holds (slots SNAPHashTable::Lookup can return) */
    uint64_t nBuckets;          /* 64-byte buckets */
    uint64_t nOverflowBuckets;  /* buckets flagged: a key homed there lives in a later bucket */
    uint64_t maxDisplacement;   /* most buckets a key lives past its home */
    uint64_t bytes;             /* HBM of the image */
    double buildMs;             /* slots upload + count + build, wall */
} snapgpu_bucket_info_t;
int snapgpu_aligner_bucket_info(const snapgpu_aligner_t *a, snapgpu_bucket_info_t *info);
/* GenomeIndex::lookupSeed + fillInLookedUpResults (GenomeIndex.cpp:971-1086, unwindowed) of n seeds
 * (seedLen ACGT bases each, concatenated) on the device, through the bucket image: mode 0 = one lane
 * per seed, each lane loading its whole line (bucket_lookup_lane: the paired kernel's lookup), 1 = the
 * whole wave per seed (bucket_lookup_wave: the aligner's and CharacterizeSeeds' in-kernel lookups),
 * 2 = one lane per seed, four lanes per line (bucket_lookup_quad: seed_lookup_kernel's lookup), run
 * on waves with a scattered half of their lanes active.  out[6 i ..]: hits forward, hits RC,
 * hash of the forward hits, of the RC hits (acc = acc * 1000003 + hit, list order, mod 2^64),
 * first forward hit, first RC hit (~0 when none); lines[i] = bucket lines loaded. */
int snapgpu_aligner_lookup_seeds(snapgpu_aligner_t *a, const char *seedBases, uint64_t n, int mode, uint64_t *out,
                                 uint32_t *lines);

/* HBM streaming-copy ceiling (diagnostic): best-of-3 time (ms) of copy_peak_kernel reading
 * `bytes` and writing `bytes` with 16-byte vector accesses. */
int snapgpu_copy_peak(snapgpu_aligner_t *a, uint64_t bytes, double *ms);

/* Self-test of the device-timeout path (diagnostic, needs no GPU): a wait that times out must
 * fail with SNAPGPU_EDEVICE, mark the aligner failed, and free no device buffer afterwards.
 * Returns 0 when the path behaves. */
int snapgpu_selftest_timeout_path(void);

/* ------------------------------------------------------------------ paired-end
 * ChimericPairedEndAligner::align (ChimericPairedEndAligner.cpp:56-126) over
 * IntersectingPairedEndAligner::align (IntersectingPairedEndAligner.cpp:142-753), constructed as
 * PairedAligner.cpp:462-482 does.  Defaults = the paired CLI's (AlignerOptions.cpp:73-77,
 * PairedAligner.cpp:57-58, 231-235, IntersectingPairedEndAligner.h:32-33). */
typedef struct snapgpu_paired_params {
    uint32_t maxHits;              /* -h: maxHits of the chimeric single-end fallback, default 16000 */
    uint32_t maxK;                 /* -d: maxDist, default 15 */
    uint32_t maxSeedsToUse;        /* -n: default 8 (0 => seedCoverage) */
    uint32_t extraSearchDepth;     /* default 2 */
    uint32_t minSpacing;           /* -s min, default 50 */
    uint32_t maxSpacing;           /* -s max, default 1000 */
    uint32_t maxBigHits;           /* -H intersectingAlignerMaxHits, default 16000 */
    uint32_t maxCandidatePoolSize; /* -mcp, default 1000000 */
    uint32_t maxReadSize;          /* MAX_READ_LENGTH (Read.h:45), default 500 */
    uint32_t forceSpacing;         /* -f, default 0 */
    double   seedCoverage;         /* used iff maxSeedsToUse == 0 */
} snapgpu_paired_params_t;

/* PairedAlignmentResult (PairedEndAligner.h:31-55) plus counters.  Fields an aligner leaves
 * unwritten keep the pre-state {status NotFound, location 0xffffffff, direction 0, score -1, mapq 0}. */
typedef struct snapgpu_pair_result {
    uint32_t location[2];
    int32_t  score[2];
    int32_t  mapq[2];
    uint8_t  status[2];            /* SNAPGPU_NOT_FOUND .. */
    uint8_t  direction[2];
    uint8_t  fromAlignTogether;
    uint8_t  alignedAsPair;
    uint16_t flags;                /* SNAPGPU_PFLAG_* */
    uint32_t nLocationsScored;     /* IntersectingPairedEndAligner::getLocationsScored() delta */
    uint32_t nSingleScored;        /* the fallback BaseAligner's getLocationsScored() delta */
    uint32_t popularSeedsSkipped;  /* both reads' popular seeds (the MAPQ input, :741) */
    uint32_t writtenBy;            /* routing (diagnostic): the intersecting pass that wrote the record --
                                      1 pass 1 (<128>), 2 pass 1b (<256>), 3 pass 2 (<512>), 4 pass 3
                                      (the reference's pools); 0 for a pair whose mates are both < 50 */
    double   probabilityOfAllPairs;   /* the intersecting aligner's MAPQ inputs (align()'s locals) */
    double   probabilityOfBestPair;
} snapgpu_pair_result_t;   /* 64 bytes */
#define SNAPGPU_PFLAG_POOL_EXHAUSTED 0x01   /* the reference soft_exits ("Ran out of ... pool entries") */
#define SNAPGPU_PFLAG_READ_TOO_LONG  0x02   /* the reference soft_exits (IntersectingPairedEndAligner.cpp:211-215) */
#define SNAPGPU_PFLAG_DEFERRED       0x04   /* left pass 1: aligned by the long-read pass or the large-pool pass */
#define SNAPGPU_PFLAG_MAPQ_FIXED     0x08   /* MAPQ re-derived on the host (threshold case) */
#define SNAPGPU_PFLAG_NUL_BYTE       0x10   /* a read of the pair holds a 0x00 byte inside its length (a
                                               corrupted upload; see SNAPGPU_FLAG_NUL_BYTE) */

void snapgpu_paired_params_default(snapgpu_paired_params_t *p);
typedef struct snapgpu_paired_aligner snapgpu_paired_aligner_t;
/* NULL (and snapgpu_last_error) without a HIP device: there is no CPU fallback. */
snapgpu_paired_aligner_t *snapgpu_paired_aligner_create(int device, const snapgpu_index_t *idx,
                                                        const snapgpu_paired_params_t *p);
void snapgpu_paired_aligner_free(snapgpu_paired_aligner_t *pa);
/* ChimericPairedEndAligner::align for pair i = (reads0[i], reads1[i]), every i, in order. */
int snapgpu_paired_align_batch(snapgpu_paired_aligner_t *pa, const snapgpu_reads_t *reads0,
                               const snapgpu_reads_t *reads1, snapgpu_pair_result_t *out);
/* IntersectingPairedEndAligner::align alone (no single-end fallback), for parity tests. */
int snapgpu_paired_intersect_batch(snapgpu_paired_aligner_t *pa, const snapgpu_reads_t *reads0,
                                   const snapgpu_reads_t *reads1, snapgpu_pair_result_t *out);
/* The single-end BaseAligner the chimeric fallback uses (maxHits, maxK, seeds of the params). */
snapgpu_aligner_t *snapgpu_paired_aligner_single(snapgpu_paired_aligner_t *pa);
/* Test accessor (as snapgpu_aligner_debug_grids): out[0] compute units; the resident workgroups per CU
 * and the grid of the pair kernel for reads up to 128 bases (out[1], out[2]), up to 256 bases (out[3],
 * out[4]: capped at out[2], whose pools it uses) and up to 512 bases (out[5], out[6]); out[7] the grid
 * of the pass over the reference's whole pools (at most out[6], halved until its pools fit 8 GB).
 * SNAPGPU_PAIRED_GRID caps every grid. */
int snapgpu_paired_aligner_debug_grids(const snapgpu_paired_aligner_t *pa, uint32_t out[8]);

/* ------------------------------------------------------------ SAM text of read pairs
 * The two lines of every pair as the paired writer prints them (SimpleReadWriter::writePair,
 * ReadWriter.cpp:133-217, over SAMFormat::writeRead with a mate, SAM.cpp:914-973), without
 * transcriptome CIGARs.  With locs[e] = location[e], or invalid where status[e] is SNAPGPU_NOT_FOUND,
 * the end written first is end 1 when locs[0] > locs[1] and end 0 otherwise; output record 2q + w is
 * the w-th written end of pair q (FLAG 0x40 for w = 0, 0x80 for w = 1).  "/1" and "/2" are dropped
 * from the two ids as writePair does; the batches' own ids and clip state (snapgpu_reads_clip) are
 * used.  The CIGAR arrays have 2n rows: row 2q + e is end e of pair q (editDistance -1 = "*"), as
 * snapgpu_cigar_batch gives them for locs[e] and direction[e].  Size contract as snapgpu_sam_format.
 * SNAPGPU_EINVAL for batches that differ in n or carry no ids, for a read whose unclipped length
 * exceeds 1024 bases, and for nOps > SNAPGPU_CIGAR_MAX_OPS.  Runs the product path's line writer on the
 * host threads. */
int snapgpu_sam_format_pairs(const snapgpu_index_t *idx, const snapgpu_reads_t *reads0, const snapgpu_reads_t *reads1,
                             const snapgpu_pair_result_t *results, const int32_t *editDistance, const uint32_t *nOps,
                             const uint32_t *ops, const char *readGroup, char *out, uint64_t cap, uint64_t *used);
/* The byte length of each of the 2n lines snapgpu_sam_format_pairs prints (lineLengths: 2n entries). */
int snapgpu_sam_pair_line_lengths(const snapgpu_index_t *idx, const snapgpu_reads_t *reads0,
                                  const snapgpu_reads_t *reads1, const snapgpu_pair_result_t *results,
                                  const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                                  const char *readGroup, uint32_t *lineLengths);
/* The same text made on the device from the pair batch the last snapgpu_paired_align_batch /
 * snapgpu_paired_intersect_batch left resident (both ends' bases and qualities stay in device
 * memory until the next of those calls, which makes the CIGARs and the text below stale).
 *
 * snapgpu_paired_cigar_resident: uploads the caller's final pair records (after the chimeric
 * fallback; 64 bytes per pair) and queues the CIGAR kernel for both ends at locs[e] and
 * direction[e] over the resident bases; the reads are not uploaded again.  useM: 'M' for '=' and 'X'.
 * `results` must hold one record for every pair of the resident batch (the call takes no count).  A read
 * over 512 bases would get edit distance -1 and CIGAR "*" here, where snapgpu_cigar_batch refuses it;
 * the pair kernels refuse such reads before a batch is resident.
 * snapgpu_paired_cigar_download waits and reads back the 2n rows (ops: 2n * SNAPGPU_CIGAR_MAX_OPS).
 *
 * snapgpu_paired_sam_resident: uploads the batches' ids and clip state and queues the formatter
 * over the 2n records with the uploaded records and the CIGAR rows on the device.  SNAPGPU_EINVAL
 * with no batch resident, with no snapgpu_paired_cigar_resident behind it, and for batches that
 * differ from the resident one in n, totalBytes or lengths.  snapgpu_paired_sam_download waits and
 * copies the text out (size contract as snapgpu_sam_format; SNAPGPU_EDEVICE if a line does not end
 * where the length pass placed it).  snapgpu_paired_sam_last_ms: the CIGAR pass and the formatter's
 * kernels between HIP events, and the download's wall time, of the last calls.
 *
 * Everything is queued on the paired aligner's stream: the next align call's copies wait for it. */
/* Pairs of the resident batch, 0 when there is none: the records snapgpu_paired_cigar_resident reads, half the
 * rows snapgpu_paired_cigar_download writes. */
uint64_t snapgpu_paired_resident_pairs(const snapgpu_paired_aligner_t *pa);
int snapgpu_paired_cigar_resident(snapgpu_paired_aligner_t *pa, const snapgpu_pair_result_t *results, int useM);
int snapgpu_paired_cigar_download(snapgpu_paired_aligner_t *pa, int32_t *editDistance, uint32_t *nOps, uint32_t *ops);
int snapgpu_paired_sam_resident(snapgpu_paired_aligner_t *pa, const snapgpu_reads_t *reads0,
                                const snapgpu_reads_t *reads1, const char *readGroup);
int snapgpu_paired_sam_download(snapgpu_paired_aligner_t *pa, char *out, uint64_t cap, uint64_t *used);
int snapgpu_paired_sam_last_ms(snapgpu_paired_aligner_t *pa, double *cigarMs, double *kernelMs, double *downloadMs);
/* The batch form: snapgpu_sam_format_pairs's arguments (idx: the paired aligner's index, or NULL)
 * uploaded, formatted by the same kernels and downloaded.  Byte-identical to snapgpu_sam_format_pairs.
 * It leaves the resident batch and its CIGAR rows alone; a resident text has to be made again. */
int snapgpu_sam_format_pairs_gpu(snapgpu_paired_aligner_t *pa, const snapgpu_index_t *idx,
                                 const snapgpu_reads_t *reads0, const snapgpu_reads_t *reads1,
                                 const snapgpu_pair_result_t *results, const int32_t *editDistance,
                                 const uint32_t *nOps, const uint32_t *ops, const char *readGroup, char *out,
                                 uint64_t cap, uint64_t *used);

/* ------------------------------------------------------------ BAM records of read pairs
 * The two uncompressed BAM records of every pair as the paired writer appends them
 * (SimpleReadWriter::writePair over BAMFormat::writeRead with a mate, Bam.cpp:596-790), without
 * transcriptome CIGARs: the arguments, the record order (record 2q + w is the w-th written end), the
 * flags, the "/1" "/2" trim and the refusals of snapgpu_sam_format_pairs.  Where a record differs from
 * the SAM line of the same end: the QNAME is the whole trimmed id (not cut at the first space), and
 * an id of more than 254 bytes after the trim is refused (SNAPGPU_EINVAL); refID / next_refID are
 * piece indices, an unmapped end takes its mate's refID / pos, next_refID / next_pos are the record's
 * own where the mate is unmapped, all four are -1 with both unmapped; tlen is the SAM TLEN truncated
 * to 32 bits; bin comes from the reference span of the ops (l_seq without ops), reg2bin(matePos - 1,
 * matePos) for an unmapped end with a mapped mate, reg2bin(-1, 0) otherwise; SEQ and QUAL cover the
 * whole unclipped read.  NM: an end with a location writes its own editDistance (also -1), an end
 * without one repeats the NM of the record written before it, the first such records of a batch
 * nmCarryIn (0 at the start of a run); *nmCarryOut (may be NULL) = the NM of the last record, the next
 * batch's nmCarryIn.  No BGZF, no header (snapgpu_bam_header, snapgpu_bgzf_compress take the records).
 * Size contract as snapgpu_bam_format.  The bytes do not depend on the host thread count. */
int snapgpu_bam_format_pairs(const snapgpu_index_t *idx, const snapgpu_reads_t *reads0, const snapgpu_reads_t *reads1,
                             const snapgpu_pair_result_t *results, const int32_t *editDistance, const uint32_t *nOps,
                             const uint32_t *ops, const char *readGroup, int32_t nmCarryIn, int32_t *nmCarryOut,
                             char *out, uint64_t cap, uint64_t *used);
/* The byte size (block_size + 4) of each of the 2n records snapgpu_bam_format_pairs writes. */
int snapgpu_bam_pair_record_lengths(const snapgpu_index_t *idx, const snapgpu_reads_t *reads0,
                                    const snapgpu_reads_t *reads1, const snapgpu_pair_result_t *results,
                                    const int32_t *editDistance, const uint32_t *nOps, const uint32_t *ops,
                                    const char *readGroup, uint32_t *recordLengths);
/* The coordinate-sort key of each of the 2n records of n pair results, in write order
 * (BAMFormat::getSortInfo, Bam.cpp:474-495): the genome location of the record's own refID / pos where
 * both are >= 0, else that of next_refID / next_pos by the same test, else UINT32_MAX.  The sorted device
 * calls below write the records in the stable order of these keys. */
int snapgpu_bam_pair_sort_keys(const snapgpu_index_t *idx, uint64_t n, const snapgpu_pair_result_t *results,
                               uint32_t *keys);
/* The same records encoded on the device from the resident pair batch, after
 * snapgpu_paired_cigar_resident (see the SAM calls above; the same checks of the batches against the
 * resident one, the same stream).  Only the ids, the clip arrays, the piece offsets and the read
 * group are uploaded.  The _sorted form writes the records in coordinate order; the NM carry runs over
 * write order in both (the reference's writer runs before its sort).  The records have their own
 * output buffers: snapgpu_paired_sam_resident and snapgpu_paired_bam_resident on one batch do not
 * disturb each other.  A new align call makes the records stale.
 * snapgpu_paired_bam_download waits and copies the records out (size contract as
 * snapgpu_bam_format; SNAPGPU_EDEVICE if a record's block_size is not the size the scan gave it);
 * *nmCarryOut (may be NULL) = the NM of the last record in write order.
 * snapgpu_paired_bam_order_download: order[j] = the write-order index (2q + w) of the j-th record of
 * the sorted output, 2n entries; SNAPGPU_EINVAL unless the last resident call was the sorted one.
 * snapgpu_paired_bam_last_ms: the encoder's kernels between HIP events and the download's wall time. */
int snapgpu_paired_bam_resident(snapgpu_paired_aligner_t *pa, const snapgpu_reads_t *reads0,
                                const snapgpu_reads_t *reads1, const char *readGroup, int32_t nmCarryIn);
int snapgpu_paired_bam_resident_sorted(snapgpu_paired_aligner_t *pa, const snapgpu_reads_t *reads0,
                                       const snapgpu_reads_t *reads1, const char *readGroup, int32_t nmCarryIn);
int snapgpu_paired_bam_download(snapgpu_paired_aligner_t *pa, char *out, uint64_t cap, uint64_t *used,
                                int32_t *nmCarryOut);
int snapgpu_paired_bam_order_download(snapgpu_paired_aligner_t *pa, uint32_t *order);
int snapgpu_paired_bam_last_ms(snapgpu_paired_aligner_t *pa, double *kernelMs, double *downloadMs);
/* The batch form: snapgpu_bam_format_pairs's arguments (idx: the paired aligner's index, or NULL)
 * uploaded, encoded by the same kernels and downloaded.  sorted != 0: in coordinate order, and order
 * (may be NULL) receives the 2n write-order indices.  Byte-identical to snapgpu_bam_format_pairs (and
 * its stable reorder by snapgpu_bam_pair_sort_keys).  It leaves the resident batch, its CIGAR rows and
 * its SAM text alone; resident records have to be made again. */
int snapgpu_bam_format_pairs_gpu(snapgpu_paired_aligner_t *pa, const snapgpu_index_t *idx,
                                 const snapgpu_reads_t *reads0, const snapgpu_reads_t *reads1,
                                 const snapgpu_pair_result_t *results, const int32_t *editDistance,
                                 const uint32_t *nOps, const uint32_t *ops, const char *readGroup, int32_t nmCarryIn,
                                 int32_t *nmCarryOut, char *out, uint64_t cap, uint64_t *used, int sorted,
                                 uint32_t *order);

/* ------------------------------------------- RNA seed census
 * BaseAligner::CharacterizeSeeds (BaseAligner.cpp:206-508) on the GPU: the seeds of AlignRead's
 * order until numSeeds directions applied (or the wrap runs out), every hit of a side that is
 * not popular recorded as (read-start location implied by the hit, seed offset).  The
 * reference returns two std::map<unsigned, std::set<unsigned>> (map = forward, mapRC = RC);
 * here each map entry is one run record, forward runs first, then RC runs, locations ascending
 * (the maps' iteration order).  The caller's aligner supplies the index (its HBM upload); the
 * scan parameters are those of the partial aligner PairedAligner.cpp:518-527 constructs. */
typedef struct snapgpu_seed_run {
    uint32_t location;     /* map key */
    uint16_t minOffset;    /* *set.begin(): smallest seed offset (forward-read coordinates) */
    uint16_t maxOffset;    /* *set.rbegin() */
    uint16_t count;        /* set.size() */
    uint8_t  direction;    /* 0: map, 1: mapRC */
    uint8_t  reserved;
} snapgpu_seed_run_t;      /* 12 bytes */
typedef struct snapgpu_seed_runs {
    uint64_t n;                 /* reads scanned */
    uint64_t *start;            /* [n + 1]: read i's runs are runs[start[i] .. start[i + 1]) */
    uint32_t *nForward;         /* [n]: how many of them are forward (map) runs */
    uint32_t *flags;            /* [n]: SNAPGPU_FLAG_READ_TOO_LONG (the reference exits), SNAPGPU_FLAG_TOO_MANY_NS */
    snapgpu_seed_run_t *runs;
    uint64_t nRuns;
} snapgpu_seed_runs_t;
typedef struct snapgpu_charseeds_params {
    uint32_t maxHits;              /* 300 (PairedAligner.cpp:520) */
    uint32_t maxK;                 /* the paired maxDist, 15: reads with more Ns are skipped */
    uint32_t numSeeds;             /* 12 (PairedAligner.cpp:523) */
    uint32_t maxReadSize;          /* 500 */
    uint32_t explorePopularSeeds;  /* 0 */
    uint32_t reserved;
} snapgpu_charseeds_params_t;
void snapgpu_charseeds_params_default(snapgpu_charseeds_params_t *p);
/* readList: indices into reads of the reads to scan (NULL: all, nList ignored).  Needs
 * (numSeeds + 1) * maxHits <= 4096 and maxReadSize <= 512.  NULL on error (snapgpu_last_error). */
snapgpu_seed_runs_t *snapgpu_characterize_seeds(snapgpu_aligner_t *a, const snapgpu_reads_t *reads,
                                                const uint64_t *readList, uint64_t nList,
                                                const snapgpu_charseeds_params_t *p);
void snapgpu_seed_runs_free(snapgpu_seed_runs_t *runs);

/* --------------------------------------- RNA paired-end product path
 * PairedAlignerContext::runIterationThread (SNAPLib/PairedAligner.cpp:405-689) batched on the
 * GPU -- what `snap-rna paired <genome> <transcriptome> <gtf> r1.fq r2.fq` computes per pair:
 * Read::clip, the length / N / quality pre-filter (:555-575), transcriptome AlignRead of each
 * read with 1000-hit export (:584-614), the genome ChimericPairedEndAligner (:625),
 * AlignmentFilter::AddAlignment / Filter (AlignmentFilter.cpp:140-214, 302-739) with
 * FindPartialMatches' CharacterizeSeeds on the GPU (:957-1037), forceSpacing and the MAPQ
 * halving (:648-663), the SAM pair records (ReadWriter.cpp:133-217, SAM.cpp:804-1153: GPU
 * CIGARs, insertSpliceJunctions for transcriptome records) and the GTF read counts
 * (GTFReader::IncrementReadCount, GTFReader.cpp:1409-1611; snapgpu_gtf_write_counts writes
 * them).  Not built: the contamination database (-x) and GTFReader::AnalyzeReadIntervals
 * (the interval report UnalignedRead and the *chromosomalPair calls feed). */
typedef struct snapgpu_rna_paired_options {
    int32_t  clipping;               /* ReadClippingType, default 3 (AlignerOptions.cpp:48) */
    uint32_t confDiff;               /* -c, default 2 */
    uint32_t maxDist;                /* -d, default 15 (filter cut-off and the partial aligner's maxK) */
    uint32_t minSpacing, maxSpacing; /* -s, default 50 1000 */
    uint32_t forceSpacing;           /* -fs */
    float    minPercentAbovePhred;   /* -fp, default 90 */
    uint32_t minPhred;               /* -fm, default 20 */
    uint32_t phredOffset;            /* -fo, default 33 */
    uint32_t useM;                   /* -M */
    uint32_t maxHitsToGet;           /* transcriptome multi-hits per read, 1000 (PairedAligner.cpp:584) */
    uint32_t ignoreMismatchedIDs;    /* -I (else mismatched ids fail the call: the reference exits) */
    const char *readGroup;           /* default "FASTQ" */
    const char *commandLine;         /* @PG CL: */
    const char *version;             /* @PG VN: */
    /* -ct: the contamination database (PairedAligner.cpp:487-505, 632-645): pairs the filter left
     * NotFound on both ends go through this paired aligner (the genome one's parameters); a pair
     * it aligns on both ends adds both ends to `contaminants` (both NULL: none) */
    struct snapgpu_paired_aligner *contaminationAligner;
    struct snapgpu_contaminants *contaminants;
    uint32_t sortOutput;             /* -so: as snapgpu_single_options_t.sortOutput */
} snapgpu_rna_paired_options_t;
void snapgpu_rna_paired_options_default(snapgpu_rna_paired_options_t *o);

typedef struct snapgpu_rna_pair_result {   /* PairedAlignmentResult after the filter (PairedEndAligner.h:31-55) */
    uint32_t location[2];      /* 0xffffffff when NotFound (the SAM writer's view) */
    uint32_t tlocation[2];     /* transcriptome location of a transcriptome record */
    int32_t  score[2];
    int32_t  mapq[2];
    uint8_t  status[2];
    uint8_t  direction[2];
    uint8_t  isTranscriptome[2];
    uint8_t  fromAlignTogether, alignedAsPair;
    uint8_t  useful;           /* passed the pre-filter */
    uint8_t  reserved[7];
} snapgpu_rna_pair_result_t;   /* 48 bytes */

typedef struct snapgpu_rna_paired_stats {
    uint64_t totalPairs, usefulPairs, singleHits, multiHits, notFound, transcriptomeRecords;
    uint64_t partialPairs, partialMatches, seedRuns;   /* FindPartialMatches scans, hits, CharacterizeSeeds runs */
    double alignMs, filterMs, seedMs, cigarMs, writeMs, wallMs;
    double prepMs;     /* clipping, ID check, pre-filter, batch views (before alignMs) */
    double countMs;    /* spacing / MAPQ adjustments and the GTF read counts (after seedMs) */
    uint64_t subBatches;   /* pipelined sub-batches (SNAPGPU_RNA_SUBBATCH pairs each; default: one): the
                              stage times above are sums over them and overlap one another in wallMs */
    double cigarGpuMs;  /* of cigarMs: the CIGAR batches (genome and transcriptome threads) */
    double spliceMs;    /* of cigarMs: insertSpliceJunctions of the transcriptome records */
    uint64_t countedPairs;  /* GTFReader::IncrementReadCount (pair form) events applied: the intragene
                               SingleHit pairs (AlignmentFilter.cpp:302-740) */
} snapgpu_rna_paired_stats_t;

/* pairedAligner: the genome aligner (snapgpu_paired_aligner_create with the paired CLI defaults);
 * transcriptomeAligner: a BaseAligner over the transcriptome index (maxHits 16000, maxK 15,
 * 8 seeds); reads0 / reads1 FASTQ batches with ids, clipped here.  samPath (or NULL) receives the
 * header and two lines per pair in input order (BAM records when it ends in ".bam"); out (or NULL)
 * one record per pair; the gtf's read counters are advanced (all of the batch's count events, or
 * none when one names an unknown transcript or gene). */
int snapgpu_rna_paired_align(snapgpu_paired_aligner_t *pairedAligner, snapgpu_aligner_t *transcriptomeAligner,
                             snapgpu_gtf_t *gtf, snapgpu_reads_t *reads0, snapgpu_reads_t *reads1,
                             const snapgpu_rna_paired_options_t *opt, const char *samPath,
                             snapgpu_rna_pair_result_t *out, snapgpu_rna_paired_stats_t *stats);
/* GTFReader::WriteReadCounts (GTFReader.cpp:1710-1772): <prefix>.{transcript,gene,junction}_{id,name}
 * .counts.txt from the gtf's read counters; snapgpu_gtf_reset_counts zeroes them. */
int snapgpu_gtf_write_counts(const snapgpu_gtf_t *gtf, const char *prefix);
int snapgpu_gtf_reset_counts(snapgpu_gtf_t *gtf);

/* MAPQ (mapq.h:32-65) as the host computes it; exported for tests. */
int snapgpu_compute_mapq(double pAll, double pBest, int score, int popularSeedsSkipped);

const char *snapgpu_last_error(void);
int snapgpu_abi_version(void);
/* This rank's host thread budget, which every host stage of the library stays within: the CPUs of
 * the affinity mask, capped by the cgroup CPU quota, divided by LOCAL_WORLD_SIZE (the ranks of the
 * node); SNAPGPU_HOST_THREADS overrides.  Read once per process.  (The reference takes `-t`,
 * ParallelTask.h:104-161.) */
int snapgpu_host_threads(void);

#ifdef __cplusplus
}
#endif
#endif /* SNAPGPU_H */
