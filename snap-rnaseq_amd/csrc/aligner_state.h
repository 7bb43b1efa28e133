// aligner_state.h -- what the aligner's translation units share and nobody else sees: the state
// behind snapgpu_aligner_t and snapgpu_device_reads_t, the grow-only device buffer, the base of the
// output chain's stage states, and the host helpers every entry point uses.  Included by aligner.hip
// (the align kernels, the pass scheduler, create / free), output_chain.hip (SAM, BAM, duplicate
// marking, BGZF, BAI), fastq_upload.hip (FASTQ parse, BGZF inflate) and paired_output.hip (the paired
// aligner's CIGARs and SAM text); everything else goes through the snapgpu_internal_* accessors
// (internal.h).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "align_device.h"
#include "bai.h"
#include "dupmark.h"
#include "internal.h"
#include "sam_format.h"

#define HIPCHK(x)                                                                       \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                         \
            snapgpu::setError(std::string(#x) + ": " + hipGetErrorString(e_));          \
            return SNAPGPU_EDEVICE;                                                     \
        }                                                                               \
    } while (0)
// inside a loop whose exit path cleans up (sets rc and leaves the enclosing loop)
#define HIPBRK(x)                                                                       \
    if (hipError_t e_ = (x); e_ != hipSuccess) {                                        \
        snapgpu::setError(std::string(#x) + ": " + hipGetErrorString(e_));              \
        rc = SNAPGPU_EDEVICE;                                                           \
        break;                                                                          \
    }
#define HIPCHKN(x)                                                                      \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                         \
            snapgpu::setError(std::string(#x) + ": " + hipGetErrorString(e_));          \
            return nullptr;                                                             \
        }                                                                               \
    } while (0)

// One execution lane = one HIP stream with what the align passes of a pass set need to run
// beside the other lane: its own element arenas (persistent waves index them by blockIdx) and
// lookup statistics.  Lane 0 serves the resident API (snapgpu_reads_upload /
// snapgpu_align_resident); snapgpu_align_batch alternates chunks over both lanes so one chunk's
// copies and host tail overlap the other chunk's kernels, and the second lane's align kernel
// fills the first one's tail.  The front stage of every pass set (counter clear, record
// pre-fill, pass 0, order_long_kernel, the simple pass) runs on the aligner's one front stream,
// a chunk or two ahead of the lanes; it writes only per-chunk buffers (ChunkSlot, EvSet).
// One chunk's input/output staging of the pipelined snapgpu_align_batch and the buffers its
// front stage writes.  Two per lane: the H2D of a lane's next chunk (on the aligner's copy stream)
// and its front stage run while the lane's current chunk is still in its align kernels, so the
// lane's next align kernel can start the moment the current one frees wave slots.
struct ChunkSlot {
    char *dBases = nullptr, *dQuals = nullptr;  // device inputs
    uint64_t *dOffsets = nullptr;
    uint32_t *dLengths = nullptr;
    uint32_t *dDefer = nullptr;                 // pass-1 / pass-2 defers, arena overflows
    snapgpu_result_t *dOut = nullptr;
    sgk::SeedRec *dSeeds = nullptr;
    uint64_t *hOffsets = nullptr;               // pinned staging
    uint32_t *hLengths = nullptr;
    snapgpu_result_t *hOut = nullptr;
    hipEvent_t h2d = nullptr;                   // inputs on the device (copy stream)
    hipEvent_t done = nullptr;                  // records back in host memory (lane stream)
    bool pending = false;
    uint64_t seq = 0, chunkBegin = 0, chunkN = 0, chunkEv = 0;
    snapgpu_result_t *chunkOut = nullptr;       // the caller's record array of the pending chunk
};

struct ExecLane {
    hipStream_t stream = nullptr;
    void *arena = nullptr;                     // main passes: arenaCap elements per wave
    void *bigArena = nullptr;                  // big-arena pass: arenaElems per wave (only when arenaCap < arenaElems)
    unsigned long long *lookupStats = nullptr; // seed_lookup_kernel: [256][4] seeds, probes, overflow counts (per call)
    hipEvent_t done = nullptr;                 // scratch event: waitLane, cross-lane ordering
    // chunk buffers of the pipelined snapgpu_align_batch (grown on demand)
    uint64_t capReads = 0, capBytes = 0;
    ChunkSlot slot[2];
    uint32_t nextSlot = 0;
    unsigned long long *hLookupStats = nullptr; // pinned copy of lookupStats
};

// Timing events of one pass set (one chunk), its device work counters and their pinned copy.
struct EvSet {
    // front stream: 3 before pass 0, 0 after pass 0 (and order_long_kernel), 4 after the simple
    // pass (the lane stream waits for it); lane stream: 5 before pass 1, 1 after pass 1, 2 after
    // passes 2 and 3
    hipEvent_t e[6] = {};
    // [0] pass-1 work, [1] pass-3 work, [2] pass-1 defers, [3] pass-2 work, [4] pass-2 defers,
    // [5] long reads (pass 0), [6] arena overflows, [7] big-arena pass work, [8..9] simple pass work /
    // bails, [10..11] forced-mode statistics, [12..13] simple pass reads / wide.  One per pass set:
    // the front stage clears it while the lanes' align kernels still use the earlier sets' counters.
    uint32_t *dCounter = nullptr;
    uint32_t *hCounter = nullptr;
};

// A grow-only device buffer (devGrow): a hipMalloc / hipFree pair per call costs more than most of
// the kernels here, and hipFree waits for the whole device.
struct DevBuf { void *p = nullptr; uint64_t cap = 0; };

// Bytes devGrow would newly allocate for `bytes`, 0 when they fit.
inline uint64_t growBytes(const DevBuf &b, uint64_t bytes) { return bytes <= b.cap ? 0 : bytes + bytes / 4 + 256; }

// The stages of the output chain; snapgpu_aligner::last has one entry for each.
enum Stage { kStageSam, kStageBam, kStageBgzf, kStageBai, kStageDup, kStages };

// What the state of every stage of the output chain is built on, for a resident batch's copy as
// for the aligner's batch-form one: the stage's device buffers (its own DevBuf members, listed once,
// in its constructor), its timing events and what the *_last_ms / *_pass_ms calls report.  A new
// stage derives from this, lists its buffers, and gets stageFree, stageLastMs, stagePassMs and the
// aligner's `last` entry for it.
struct StageState {
    static constexpr int kMaxEv = 8;
    const Stage stage;
    const int nEv;                    // events of ev[] the stage uses
    std::vector<DevBuf *> bufs;       // every device buffer of the stage
    hipEvent_t ev[kMaxEv] = {};       // the stage's comment says what each is recorded around
    bool ran = false;                 // the stage's output is current (a later call upstream clears it)
    bool launched = false;            // the last event was recorded: kernels may still use the buffers
    bool empty = false;               // the last call had nothing to run (n == 0, no block): no event was recorded
    double downloadMs = 0;
    StageState(Stage stage, int nEv, std::initializer_list<DevBuf *> b) : stage(stage), nEv(nEv), bufs(b) {}
    StageState(const StageState &) = delete;
};

// Device SAM formatter (sam_format.hip) state of one resident batch, or of the aligner's batch-form
// calls.
struct SamState : StageState {
    DevBuf aux;            // ids, id offsets / lengths, clip arrays, piece names, read group (one packed upload)
    DevBuf len, scans, start, sums, text, bad;
    DevBuf bases, quals;   // the reads where the unclipped extents pass the resident upload (or the batch form's reads)
    DevBuf res, ed, nOps, ops;   // batch form: records and CIGARs from the host
    // coordinate-sorted calls (samgpu::SortBuffers): keys, their sorted copy, 0 .. n - 1, the output
    // order, the lengths in that order, rocPRIM's temporary storage
    DevBuf key, keySorted, iota, order, slotLen, sortTemp;
    bool sorted = false;      // the last call was a sorted one: `order` holds its n record indices
    samline::SortArgs sortArgs{};   // samline::sortKey's per-piece tables in aux (samPrepare)
    std::vector<char> hAux;   // host copy of aux (alive while its upload may be in flight)
    uint64_t fullBytes = 0;   // bytes of bases / quals valid in `bases` / `quals` (resident: 0 = the batch's own)
    bool idsCached = false;   // aux holds the batch's own ids (reads->ids), with this read group:
    std::string cachedRg;
    bool cachedHasRg = false;
    bool cachedDevForm = false;   // ... laid out for a call without a host batch (reads == NULL): no ids, no clip arrays
    uint64_t n = 0, textBound = 0;
    // ev: before the length pass, after the check; after the length pass, after the scan; after the sort step
    // (a state built on this one may ask for more events and say what they are recorded around)
    explicit SamState(Stage stage = kStageSam, int nEv = 5)
        : StageState(stage, nEv, {&aux, &len, &scans, &start, &sums, &text, &bad, &bases, &quals, &res, &ed, &nOps, &ops,
                                  &key, &keySorted, &iota, &order, &slotLen, &sortTemp}) {}
};

// One packed upload of small host arrays (SamState::aux): 16-byte aligned pieces, each piece's
// offset known when it is added, the bytes copied later or not at all.
struct AuxPack {
    struct Piece { const void *p; uint64_t at, bytes; };
    std::vector<Piece> pieces;
    uint64_t end = 0;   // 16-byte aligned
    // `bytes` at p (null: zeros) -> their offset in the upload
    uint64_t add(const void *p, uint64_t bytes) {
        pieces.push_back({p, end, bytes});
        end = (end + bytes + 15) & ~15ull;
        return pieces.back().at;
    }
    uint64_t bytes() const { return end + 16; }   // with 16 bytes of zeros behind the last piece
    void copyTo(std::vector<char> &h) const {
        h.assign(bytes(), 0);
        for (const Piece &c : pieces)
            if (c.p && c.bytes) memcpy(h.data() + c.at, c.p, c.bytes);
    }
};

// What the download of a text stage says: the message of a failed check, a printf format over (bad,
// records, bytes, bound), and the call's name in "<call>: output buffer too small".
struct StageWords { const char *checkFmt, *call; };

// Device BAM encoder (bam_format.hip) state: the SAM formatter's buffers (its own copies: a batch's
// SAM and BAM calls do not disturb each other) and the NM carry's.
struct BamState : SamState {
    DevBuf nm, nmTiles;
    int32_t carryIn = 0;
    BamState() : SamState(kStageBam) { bufs.insert(bufs.end(), {&nm, &nmTiles}); }
};

// Device BGZF compressor (bgzf.hip) state of one resident batch, or of the aligner's batch form:
// bgzfgpu::Buffers, the batch form's copy of its input.
struct BgzfState : StageState {
    DevBuf in, slots, sizes, offs, tokens, packed, res;
    uint64_t maxBlocks = 0;   // what the last call's buffers were sized for (0: nothing to compress)
    // ran: the compressed stream is that of the batch's last BAM call
    // ev: before the compress pass, after it, after the scan, after the check
    BgzfState() : StageState(kStageBgzf, 4, {&in, &slots, &sizes, &offs, &tokens, &packed, &res}) {}
};

// Device BAI builder (bai.hip) state of one resident batch, or of the aligner's batch form: the
// passes' work area (baigpu::Layout), the index, the batch form's record starts.
struct BaiState : StageState {
    DevBuf work, out, starts;
    baigpu::Layout L{};
    uint64_t n = 0, nRef = 0, outCap = 0;
    // ran: the index is that of the batch's last BAM and BGZF calls; ev: around the passes
    BaiState() : StageState(kStageBai, baigpu::kPasses + 1, {&work, &out, &starts}) {}
};

// Device duplicate marking (dupmark.hip) state of one resident batch, or of the aligner's batch form:
// the passes' work area (dupgpu::Layout), the batch form's records and starts.
struct DupState : StageState {
    DevBuf work, in, starts;
    dupgpu::Layout L{};
    // ran: the batch's records are the marked ones of its last BAM call; ev: around the passes
    DupState() : StageState(kStageDup, dupgpu::kPasses + 1, {&work, &in, &starts}) {}
};
static_assert(baigpu::kPasses < StageState::kMaxEv && dupgpu::kPasses < StageState::kMaxEv, "StageState::ev is too short");

struct snapgpu_device_reads {
    snapgpu_aligner_t *owner = nullptr;
    char *dBases = nullptr, *dQuals = nullptr;
    uint64_t *dOffsets = nullptr;
    uint32_t *dLengths = nullptr;
    snapgpu_result_t *dOut = nullptr;
    uint32_t *dDefer = nullptr;   // pass 1 -> pass 2 read list
    sgk::SeedRec *dSeeds = nullptr;    // seed_lookup_kernel records, SEEDS_PER_READ per read
    int32_t *dCigEd = nullptr;    // cigar_kernel outputs (allocated by the first snapgpu_cigar_resident)
    uint32_t *dCigN = nullptr, *dCigOps = nullptr;
    uint64_t n = 0;
    uint32_t maxLen = 0;
    int device = 0;
    uint64_t bytes = 0;       // bases / quals bytes uploaded: the largest clipped end
    uint64_t extentHash = 0;  // of the offsets and lengths uploaded (snapgpu_sam_resident checks its batch)
    // What the device FASTQ parser leaves for the SAM / BAM calls without a host batch (reads == NULL);
    // a batch from snapgpu_reads_upload has none of it.
    bool hasIds = false;
    int clipping = 0;             // 0: no clip arrays (front / unclipped below are not used)
    char *dIds = nullptr;         // the packed ids, idTotal + 16 bytes
    char *dMeta = nullptr;        // one allocation: idStart, idLen, front, baseLen (16-byte aligned each)
    const uint64_t *dIdStart = nullptr;
    const uint32_t *dIdLen = nullptr, *dFront = nullptr, *dUnclipped = nullptr;
    char *dTail = nullptr;        // bases, then qualities, of [bytes, total): what the zeroing from `bytes` on took
    uint64_t total = 0, idTotal = 0;        // bytes of all unclipped reads, of all ids
    uint32_t maxUnclipped = 0, maxIdLen = 0;
    SamState sam;
    BamState bam;
    BgzfState bgzf;
    BaiState bai;
    DupState dup;
    StageState *stages[kStages] = {&sam, &bam, &bgzf, &bai, &dup};   // by Stage
};

// Device FASTQ parser (snapgpu_fastq_upload): the text, newline positions and per-record arrays,
// grow-only; the pinned staging of the text upload (two chunks in flight); the last call's times.
struct FastqState {
    DevBuf text, counts, tileStart, sums, nl, rec, baseStart, idStart, sums2, tot;
    void *pin[2] = {};
    hipEvent_t pinDone[2] = {};
    hipEvent_t ev[9] = {};   // 0-2 count, scan; 3-6 line starts, record pass, scans; 7-8 copy pass
    bool ran = false;
    double uploadMs = 0, kernelMs = 0, downloadMs = 0;
    double passMs[6] = {};   // count, scan, line starts, records, scans, copy (snapgpu_internal_fastq_pass_ms)
    double arriveKernelMs = 0;   // kernels that brought the text (the BGZF form's inflate kernel)
};

// Device BGZF inflater (inflate.hip): the compressed stream, its member table, the members'
// statuses with the lowest refused index after them, and the batch form's output, grow-only;
// the last call's times (snapgpu_bgzf_inflate_last_ms).
struct InflateState {
    DevBuf in, members, status, out;
    hipEvent_t ev[2] = {};
    int waves = 0;           // waves of the inflate kernel: inflategpu::kWavesPerCu per CU
    bool ran = false;
    double uploadMs = 0, kernelMs = 0, downloadMs = 0;
};

struct snapgpu_aligner {
    int device = 0;
    const snapgpu_index_t *idx = nullptr;
    snapgpu_aligner_params_t p{};
    uint32_t *dOverflow = nullptr, *dPieces = nullptr;
    // the seed tables' bucket image (bucket_table.h), built on the device at creation
    uint4 *dBuckets = nullptr;
    uint64_t *dBucketBase = nullptr;
    uint32_t *dBucketCount = nullptr;
    snapgpu_bucket_info_t bucketInfo{};
    char *dGenomeAlloc = nullptr;
    sgk::GPlane *dGPlanes = nullptr;   // genome bit planes (KArgs::gpl)
    const char *dGenome = nullptr;
    sgk::DevTables *dTab = nullptr;
    ExecLane lane[2];
    std::vector<EvSet> evs;       // one per pass set of the current call (grown on demand)
    uint64_t nEvUsed = 0;
    // Pass sets of the two lanes run concurrently: the second lane's waves fill the tail of the
    // first one's persistent kernel (the last, heavy reads of a launch).  SNAPGPU_OVERLAP=0 runs
    // them one after the other (copies and host tails still overlap).  With overlap, launch
    // durations overlap too: snapgpu_timing_t also carries the union of the launch intervals.
    bool overlapKernels = true;
    // snapgpu_align_batch_submit: chunks of consecutive batches stream through the lanes until
    // snapgpu_align_batch_wait; timing and statistics cover that whole stream
    bool streamOpen = false;
    uint64_t nextLane = 0;
    uint64_t chunkSeq = 0;        // submission order of pipelined chunks (finished oldest first)
    hipStream_t copyStream = nullptr;   // H2D of the pipelined chunks
    // CIGAR (cigar_kernel) and seed-census (charseeds.hip) calls: their own stream and buffers, so a
    // host thread can run them while another thread's align call keeps the lanes busy (the RNA
    // paired path's sub-batch pipeline); a caller serialises them among themselves
    hipStream_t sideStream = nullptr;
    // the front stage of every pass set, both lanes' (launch_passes): one stream, so the front
    // stages run in submission order -- its small kernels take the wave slots a lane's persistent
    // kernel frees in its tail without queueing behind the other lane's passes 2 / 3 and record copy
    // (normal priority; SNAPGPU_FRONT_PRIORITY=1: the device's highest)
    hipStream_t frontStream = nullptr;
    hipEvent_t frontDone = nullptr;     // scratch event: waitFront, lane -> front ordering
    uint32_t *dSink = nullptr;          // 64 B nobody reads (snapgpu_gather_peak's result sink)
    std::chrono::steady_clock::time_point streamStart;
    uint64_t arenaElems = 0;      // worst case per read: (maxSeeds + 2) * maxHits (+ 64)
    uint64_t arenaCap = 0;        // per wave in the main passes (= arenaElems unless that cannot fit the grid)
    int grid = 0, grid256 = 0, grid512 = 0, gridBig = 0;
    // resident workgroups per CU of each persistent kernel (resident_grid.h) behind those grids
    int perCU128 = 0, perCU256 = 0, perCU512 = 0, perCUSimple = 0, perCUCigar = 0;
    bool shortRows = false;       // pass 1 runs align_kernel<128, EXT, SHORT_ROWS>: maxK + extraSearchDepth <= SHORT_ROWS
    // snapgpu_align_batch chunk (SNAPGPU_CHUNK_READS): a streaming caller's 1M-read batches go
    // as one chunk each, alternating lanes (fewest persistent-kernel tails; A/B in
    // profiles/r02/ab/chunk_size_slots.txt); resident runs keep 2^18-read chunks over both lanes
    uint64_t chunkReads = 1u << 20;
    uint64_t residentChunk = 1u << 18;
    // forced mode: reads with at least this many elements get a radix-sorted pop order instead of
    // windowed ranks (SNAPGPU_RADIX_MIN; beyond SKCAP the ranks stage keys from HBM per window)
    uint32_t radixMin = sgk::SKCAP + 1;
    bool simplePass = true;       // simple_align_kernel ahead of pass 1 (SNAPGPU_SIMPLE_PASS=0: off)
    int gridSimple = 0;
    bool orderLong = true;        // pass 2's list longest-first (SNAPGPU_ORDER_LONG=0: pass 0's order)
    uint32_t tripRead = 0xffffffffu;   // test hook (snapgpu_aligner_debug_trip): trip the watchdog at this read
    snapgpu_timing_t timing{};
    snapgpu_aligner_stats_t stats{};
    snapgpu_device_reads_t *lastReads = nullptr;
    bool pendingTiming = false;
    uint32_t *dDiag = nullptr;    // this aligner's watchdog record (KArgs::diag)
    unsigned long long *dPhase = nullptr;   // [grid][PH_SLOTS] (SNAPGPU_PHASES=1 diagnostics)
    double timeoutSec = 0;        // SNAPGPU_TIMEOUT_S
    // A wait that timed out leaves kernels running on buffers this aligner owns: from then on
    // nothing is freed or reused (hipFree would block on the running kernel, a reuse could
    // fault it); every call fails and the process is expected to exit.
    bool failed = false;
    hipError_t (*eventQuery)(hipEvent_t) = hipEventQuery;   // test hook (snapgpu_selftest_timeout_path)
    hipEvent_t cev[2] = {};       // cigar_kernel timing
    // snapgpu_cigar_resident reads a resident batch's records (d->dOut) on the side stream; the
    // next pass set over resident reads (launch_resident: its 0xff pre-fill and the passes rewrite
    // those records) waits for this event on both lanes first
    hipEvent_t residentSideDone = nullptr;
    bool residentSidePending = false;
    int cigarGrid = 0;
    // snapgpu_align_batch_ex buffers, kept across calls: search windows, multi-hit scratch per block,
    // found counts, hit rows, compaction offsets and the packed hits
    DevBuf exSearch, exScratch, exFound, exHits, exOff, exDense;
    // snapgpu_cigar_batch (device inputs, device outputs, pinned staging of the packed inputs) and
    // the internal scratch slots of snapgpu_internal_devbuf (charseeds.hip)
    DevBuf cgIn, cgOut, aux[8];
    // snapgpu_internal_align_batch_packed: its device reads, kept (grow-only) across calls -- a
    // snapgpu_reads_upload / _free per call is ten hipMalloc / hipFree pairs, and each hipFree waits
    // for the whole device, the RNA path's concurrent genome aligner included
    snapgpu_device_reads_t *exReads = nullptr;
    uint64_t exReadsCapN = 0, exReadsCapBytes = 0;
    void *cgPin = nullptr, *cgPinOut = nullptr;
    uint64_t cgPinCap = 0, cgPinOutCap = 0;
    // the output chain (output_chain.hip): the batch forms' states, the state each stage's last call
    // used (a resident batch's or the batch form's; the *_last_ms calls read it, and
    // snapgpu_device_reads_free clears what points into the batch it frees), and the pinned staging
    // of the text download (two chunks in flight)
    SamState samBatch;
    BamState bamBatch;
    BgzfState bgzfBatch;
    BaiState baiBatch;
    DupState dupBatch;
    StageState *batchStages[kStages] = {&samBatch, &bamBatch, &bgzfBatch, &baiBatch, &dupBatch};   // by Stage
    StageState *last[kStages] = {};
    int bgzfGrid = 0;              // workgroups of the compress pass: one per CU
    void *samPin[2] = {};
    hipEvent_t samPinDone[2] = {};
    FastqState fq;      // fastq_upload.hip
    InflateState inf;
    hipStream_t stream() const { return lane[0].stream; }
};

extern std::atomic<uint64_t> g_devFrees;   // hipFree calls made by devFree (snapgpu_selftest_timeout_path)

// ---- defined in aligner.hip
// Every device free goes through here: after a timeout the aligner's buffers may still be
// in use by a running kernel, so they are left alone (see snapgpu_aligner::failed).
void devFree(const snapgpu_aligner_t *a, void *p);
void hostPinnedFree(void *p);
// b holds at least `bytes` afterwards: what is there is freed first and bytes + bytes / 4 + 256
// allocated (growBytes); cap = 0 when that fails.
hipError_t devGrow(const snapgpu_aligner_t *a, DevBuf &b, uint64_t bytes);
// Wait for an event, honouring SNAPGPU_TIMEOUT_S: on expiry the aligner is marked failed.
int waitEvent(snapgpu_aligner_t *a, hipEvent_t ev);
// Wait for everything queued on a lane's stream (an event recorded now, then waitEvent).
int waitLane(snapgpu_aligner_t *a, ExecLane &L);
// running hash of a batch's (offset, length) pairs
uint64_t extentMix(uint64_t h, uint64_t off, uint32_t len);
// cigar_kernel over n reads that are in device memory already (read r = dBases[dOffsets[r] .. +
// dLengths[r]), at explicit locations and directions, into device rows, queued on st (the caller's
// stream and timing; a's genome upload and CIGAR grid).  Reads over 512 bases get edit distance -1.
extern "C" int snapgpu_internal_cigar_device(snapgpu_aligner_t *a, hipStream_t st, const char *dBases, const uint64_t *dOffsets, const uint32_t *dLengths,
                uint64_t n, const uint32_t *dLocations, const uint8_t *dDirections, int useM, int32_t *dEd, uint32_t *dNOps,
                uint32_t *dOps);

// ---- defined in output_chain.hip
// S's buffers and events back to the runtime (neither once the aligner has failed).
void stageFree(const snapgpu_aligner_t *a, StageState &S);
// S's nEv events, created by the stage's first launch.
int stageEvents(StageState &S);
// The text stage's buffers for n records (0 < n < 2^32) and S.textBound bytes of text, grown, into
// *B (no mid events).
int textBuffers(const snapgpu_aligner_t *a, SamState &S, uint64_t n, samgpu::Buffers *B);
// The sort step's buffers of a sorted call over n records: S's, grown, into *SB (keys and done are
// left to the caller).
int sortBuffers(snapgpu_aligner_t *a, SamState &S, uint64_t n, samgpu::SortBuffers *SB);
// What follows a text stage's kernels (S.ev[1] recorded behind them, S.n records): wait for them,
// fetch start[n] and bad and compare them with S.textBound (SNAPGPU_EDEVICE, in W's words), *used =
// the bytes, then copy them to out[0 .. cap) (textDownload; SNAPGPU_EINVAL when they do not fit).
// checked(S, arg), if given, runs once the check has passed (the BAM stage's carry-out).
// S.downloadMs = the wall ms after the wait.  S.n == 0: nothing to do.
int textFinish(snapgpu_aligner_t *a, SamState &S, const StageWords &W, char *out, uint64_t cap, uint64_t *used,
               int (*checked)(SamState &, void *) = nullptr, void *arg = nullptr);
// `total` bytes at device address `text` to the caller's (pageable) buffer, in chunks through two
// pinned staging buffers: chunk k + 1 crosses PCIe while host threads copy chunk k out.
int textDownload(snapgpu_aligner_t *a, const char *text, uint64_t total, char *out);

// ---- defined in fastq_upload.hip
// The parser's and the inflater's buffers, staging and events (snapgpu_aligner_free).
void fastqStateFree(snapgpu_aligner_t *a);
