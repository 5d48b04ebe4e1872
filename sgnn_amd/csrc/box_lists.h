// Listing a face in every cell of an integer box: the count and the fill pass of the CSR lists that meshdist.hip keeps
// per grid cell and voxelize.hip per 8x8x8 brick.  The two kernels differ in how a face's box becomes a range of cells;
// what follows is this header.  The scan between the two passes is the caller's.  Integer arithmetic only.
#pragma once
#include "common.h"

// First cell and cells per axis of the box a face touches; sx == 0: nothing.
struct CellRange {
  int x0, y0, z0, sx, sy, sz;
};

constexpr int WAVE_CELLS = 256;   // a face whose range holds more cells is listed by its whole wave

// List face t in every cell (z * ny + y) * nx + x of range r: counts[cell] grows by one, and with FILL the face goes to
// refs[offsets[cell] + the count before], so the order inside a cell is the atomics'.  A lane walks a small range on its
// own; a range of more than WAVE_CELLS cells is spread over the wave, 64 consecutive cells per step.
// The routine holds a ballot: every lane of a wave must call it, a lane without a face with an empty range, and no lane
// may return before it.
template <bool FILL>
__device__ __forceinline__ void list_in_cells(CellRange r, int t, int nx, int ny,
                                              const int32_t *__restrict__ offsets, int32_t *__restrict__ counts,
                                              int32_t *__restrict__ refs) {
  auto put = [&](int c, int f) {
    const int k = atomicAdd(counts + c, 1);
    if (FILL) refs[offsets[c] + k] = f;
  };
  const int64_t total = (int64_t)r.sx * r.sy * r.sz;
  const bool big = total > WAVE_CELLS;
  if (r.sx > 0 && !big)
    for (int z = r.z0; z < r.z0 + r.sz; ++z)
      for (int y = r.y0; y < r.y0 + r.sy; ++y)
        for (int x = r.x0; x < r.x0 + r.sx; ++x) put((z * ny + y) * nx + x, t);
  unsigned long long todo = __ballot(big);
  const int lane = (int)(threadIdx.x & 63);
  while (todo) {
    const int src = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(todo));
    todo &= todo - 1;
    const int bx0 = __builtin_amdgcn_readlane(r.x0, src), by0 = __builtin_amdgcn_readlane(r.y0, src);
    const int bz0 = __builtin_amdgcn_readlane(r.z0, src), bsx = __builtin_amdgcn_readlane(r.sx, src);
    const int bsy = __builtin_amdgcn_readlane(r.sy, src), bsz = __builtin_amdgcn_readlane(r.sz, src);
    const int f = __builtin_amdgcn_readlane(t, src);
    const int64_t n = (int64_t)bsx * bsy * bsz;
    for (int64_t q = lane; q < n; q += 64) {
      const int x = (int)(q % bsx), y = (int)((q / bsx) % bsy), z = (int)(q / ((int64_t)bsx * bsy));
      put(((bz0 + z) * ny + (by0 + y)) * nx + (bx0 + x), f);
    }
  }
}
