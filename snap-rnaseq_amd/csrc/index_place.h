// index_place.h -- where a key goes in a SNAPHashTable, as text shared by the device index
// builder (index_build.hip) and a host lock-step test (tests/c/index_place_test.cpp).
//
// The CPU builder (host/index.cpp) inserts a table's keys in ascending order, each at the first
// free slot of Lookup's probe sequence (HashTable.h:74-105): home = hash(key) % size, then + p*p
// for probes 1..4, then + 1.  placeClaim reaches the same table in parallel by priority claiming:
// every slot has an owner word, initially kPlaceNone; the thread that carries the key of rank r
// (its position in ascending key order) walks r's probe sequence and does atomicMin(owner, r).
//   old > r:  the claim stands.  If old was a real rank, that key is evicted: the same thread now
//             carries it and restarts it from its own home slot.
//   old < r:  the slot belongs to a lower rank, now and for good (owners only decrease): next probe.
// No thread waits for another.  When all threads have returned, every key sits at the first slot
// of its sequence that no lower rank holds; by induction on the rank that is where sequential
// insertion puts it.  Every walk is bounded like lookupSlot's (size + kPlaceChainingDepth probes):
// an overrun is reported, never spun on.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SNAPGPU_HD __host__ __device__
#else
#define SNAPGPU_HD
#endif

namespace snapgpu {

constexpr uint32_t kPlaceNone = 0xffffffffu;      // owner word of a free slot
constexpr unsigned kPlaceChainingDepth = 5;       // kQuadraticChainingDepth (HashTable.h:115)

// SNAPHashTable::hash (HashTable.h:60-72): MurmurHash3 fmix32 (hashKey of host/internal.h).
SNAPGPU_HD inline uint32_t placeHash(uint32_t key) {
    key ^= key >> 16;
    key *= 0x85ebca6bu;
    key ^= key >> 13;
    key *= 0xc2b2ae35u;
    key ^= key >> 16;
    return key;
}

SNAPGPU_HD inline uint64_t placeHome(uint32_t key, uint64_t size) { return placeHash(key) % size; }

// The slot after slot i of a probe sequence; probes counts the steps taken from the home slot.
SNAPGPU_HD inline uint64_t placeNext(uint64_t i, uint64_t *probes, uint64_t size) {
    const uint64_t p = ++*probes;
    return p < kPlaceChainingDepth ? (i + p * p) % size : (i + 1) % size;
}

// Place the key of rank `rank` (and whatever it evicts) in a table of `size` slots.
//   atomicMinOwner(slot, r) -> the owner word's previous value, after owner = min(owner, r)
//   keyOf(r)                -> the key of rank r
// false: a walk overran its bound (more keys than slots, or a bug) -- the caller must fail.
template <class AtomicMin, class KeyOf>
SNAPGPU_HD inline bool placeClaim(uint32_t rank, uint64_t size, AtomicMin &&atomicMinOwner, KeyOf &&keyOf) {
    uint32_t r = rank;
    uint64_t i = placeHome(keyOf(r), size), probes = 0;
    for (;;) {
        const uint32_t old = atomicMinOwner(i, r);
        if (old >= r) {
            if (old == kPlaceNone || old == r) return true;
            r = old;                                  // evicted: carry it from its own home
            i = placeHome(keyOf(r), size);
            probes = 0;
            continue;
        }
        if (probes >= size + kPlaceChainingDepth) return false;
        i = placeNext(i, &probes, size);
    }
}

}  // namespace snapgpu
