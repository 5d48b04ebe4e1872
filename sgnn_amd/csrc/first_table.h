// The open-addressing "first member" table of the mesh tools: every member i of a set hashes its key to a home slot,
// the first member to reach an empty slot on the probe sequence claims it for the key, and first[slot] ends up as the
// smallest member index of that key.  Which member claims a slot depends on timing; which slot a key gets and what
// first[] holds do not.  The table has more slots than keys (sgnn_weld_slots), so every probe ends.
//
// A slot (type T, memset to 0xFF = SLOT_EMPTY; first[] to 0x7F) holds what its claimant stored: the claimant's own index
// where the keys sit in an array written before the inserts (int32: the vertex weld of mc.hip, the duplicate-face set of
// mesh_tables.hip), or the 64-bit key itself (simplify.hip's clusters, voxelize.hip's edges).  match(slot value) says
// whether a slot belongs to the caller's key.
#pragma once
#include "common.h"

// An integer triple as a key: the weld's grid cell (mc.hip calls it Cell), or the sorted vertex triple of a face.
struct Key3 {
  int x, y, z;
};
__device__ __forceinline__ bool operator==(const Key3 &a, const Key3 &b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

__device__ __forceinline__ uint64_t weld_hash(const Key3 &c) {
  uint64_t h = (uint64_t)(uint32_t)c.x * 0x9E3779B97F4A7C15ull;
  h ^= (uint64_t)(uint32_t)c.y * 0xC2B2AE3D27D4EB4Full + (h << 6) + (h >> 2);
  h ^= (uint64_t)(uint32_t)c.z * 0x165667B19E3779F9ull + (h << 6) + (h >> 2);
  h ^= h >> 29;
  return h;
}

template <typename T> constexpr T SLOT_EMPTY = (T)-1;      // all ones

// Enter member i, probing from its key's home slot h (hash % cap); claiming a slot stores `mine` in it.
template <typename T, typename Match>
__device__ __forceinline__ void first_insert(T *slot, int32_t *first, int64_t cap, int64_t h, int32_t i, T mine,
                                             Match match) {
  for (;;) {
    T cur = __hip_atomic_load(&slot[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == SLOT_EMPTY<T>) {
      const T old = atomicCAS(&slot[h], SLOT_EMPTY<T>, mine);
      cur = old == SLOT_EMPTY<T> ? mine : old;
    }
    if (match(cur)) {
      atomicMin(&first[h], i);
      return;
    }
    h = h + 1 == cap ? 0 : h + 1;
  }
}

// The slot of a key in a finished table, probing from its home slot h; -1 when the probe meets an empty slot.
// KNOWN_PRESENT: the caller entered this key itself, so the probe does not look for empty slots (and must not be used
// for a key that may be absent: it would not end).
template <bool KNOWN_PRESENT = false, typename T, typename Match>
__device__ __forceinline__ int64_t first_find(const T *slot, int64_t cap, int64_t h, Match match) {
  for (;;) {
    const T cur = slot[h];
    if (!KNOWN_PRESENT && cur == SLOT_EMPTY<T>) return -1;
    if (match(cur)) return h;
    h = h + 1 == cap ? 0 : h + 1;
  }
}
