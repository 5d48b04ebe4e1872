// Exact Euclidean feature transform of a dense seed mask and the colour gather built on it (include/sgnn_hip.h,
// "Euclidean feature transform"; rules in INTEGRATION.md section O).  Integer work only: no floating point in this
// unit.
//
// Three separable passes.  Between passes a voxel carries its partial nearest seed as packed coordinates
// f = sz << 20 | sy << 10 | sx (every axis <= 1024, so 10 bits each; -1 = no seed yet).  The partial distance is
// recomputed from the coordinates, not stored.  Packed coordinates compare like the seed's linear index, so the key
// (dist2 << 32 | f) of a candidate, minimised as ONE unsigned 64-bit integer, is "nearest, then smallest linear index":
// the tie rule of the contract, without a branch.  No candidate is the key ~0.
//
//   k_edt_rows   one wave per row (z, y), four rows per workgroup.  The seeds of a 64-voxel chunk are one __ballot,
//                kept in LDS (16 words per row at most); the nearest seed to the left / right inside the chunk is a
//                count of leading / trailing zeros of the masked ballot, and beyond the chunk it is the chunk's carry:
//                the last seed before it and the first seed after it, found by lane c for chunk c.  Equal distances
//                go left (the smaller x).
//   k_edt_axis   y or z pass.  A wave holds 64 x-adjacent voxels of one (z, y), so every load along the pass axis is
//                one coalesced row segment and the candidates at offset d are the same two rows for all lanes.  The
//                walk goes outward, d = 1, 2, .., four offsets per trip (eight independent loads), and ends, for the
//                whole wave, when no lane has d * d <= its best squared distance (<=, not <: an equal candidate at a
//                lower coordinate still has to be seen) or when d passes the reach or both ends of the axis.  Offsets
//                are clamped to the axis: a clamped offset reads a real candidate a second time, which a minimum does
//                not notice.  The four waves of a workgroup are neighbours along the pass axis and read nearly the
//                same rows (L1); the last pass writes dist2 and the linear index instead of the packed feature.
//   k_edt_fill   out[p] = colors[nearest[p]] or 0, three bytes per voxel.
//
// No per-thread array is indexed at run time and nothing goes to scratch memory.  The cap: a partial candidate beyond
// cap2 is dropped at once (the later passes only add to its distance), and no walk goes beyond reach =
// floor(sqrt(cap2)); every voxel within the cap gets what it gets without one.
#include "common.h"

namespace {

constexpr int EDT_MAX_DIM = SGNN_EDT_MAX_DIM;
constexpr int CHUNKS = EDT_MAX_DIM / 64;       // ballots per row
constexpr uint64_t NO_KEY = ~0ull;
static_assert(EDT_MAX_DIM == 1024, "three coordinates of 10 bits in one int32");

__device__ __forceinline__ int32_t edt_pack(int z, int y, int x) { return (z << 20) | (y << 10) | x; }

// key of the candidate f for the voxel (z, y, x)
__device__ __forceinline__ uint64_t edt_key(int32_t f, int z, int y, int x) {
  if (f < 0) return NO_KEY;
  const int ez = z - (f >> 20), ey = y - ((f >> 10) & 1023), ex = x - (f & 1023);
  return ((uint64_t)(uint32_t)(ez * ez + ey * ey + ex * ex) << 32) | (uint32_t)f;
}

__global__ __launch_bounds__(256) void k_edt_rows(const uint8_t *__restrict__ mask, int64_t rows, int dy, int dx,
                                                  int cap2, int32_t *__restrict__ feat) {
  __shared__ uint64_t bal[4][CHUNKS];
  __shared__ int32_t left[4][CHUNKS], right[4][CHUNKS];     // last seed before / first seed after the chunk, -1 = none
  const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * 4 + w;
  const bool live = row < rows;                              // wave-uniform; no early return: barriers below
  const int nchunks = (dx + 63) >> 6;
  const int64_t base = row * dx;
  if (live)
    for (int c = 0; c < nchunks; ++c) {
      const int x = c * 64 + lane;
      const uint64_t b = __ballot(x < dx && mask[base + x] != 0);
      if (lane == 0) bal[w][c] = b;
    }
  __syncthreads();
  if (live && lane < nchunks) {
    int l = -1, r = -1;
    for (int c = lane - 1; c >= 0 && l < 0; --c) {
      const uint64_t b = bal[w][c];
      if (b) l = c * 64 + 63 - __clzll((long long)b);
    }
    for (int c = lane + 1; c < nchunks && r < 0; ++c) {
      const uint64_t b = bal[w][c];
      if (b) r = c * 64 + __ffsll((unsigned long long)b) - 1;
    }
    left[w][lane] = l;
    right[w][lane] = r;
  }
  __syncthreads();
  if (!live) return;
  const int y = (int)(row % dy), z = (int)(row / dy);
  for (int c = 0; c < nchunks; ++c) {
    const int x = c * 64 + lane;
    if (x >= dx) break;
    const uint64_t b = bal[w][c];
    const uint64_t lo = b & (~0ull >> (63 - lane));         // seeds at lanes <= lane
    const uint64_t hi = b & (~0ull << lane);                // seeds at lanes >= lane
    const int l = lo ? c * 64 + 63 - __clzll((long long)lo) : left[w][c];
    const int r = hi ? c * 64 + __ffsll((unsigned long long)hi) - 1 : right[w][c];
    int sx = -1;
    if (l >= 0 && (r < 0 || x - l <= r - x)) sx = l;         // equal distances: the smaller x
    else if (r >= 0) sx = r;
    int32_t f = -1;
    if (sx >= 0) {
      const int e = x - sx;
      if (e * e <= cap2) f = edt_pack(z, y, sx);
    }
    feat[base + x] = f;
  }
}

// AXIS 1: along y; AXIS 0: along z.  fin holds the result of the pass before.  LAST: write dist2 and nearest.
template <int AXIS, bool LAST>
__global__ __launch_bounds__(256) void k_edt_axis(const int32_t *__restrict__ fin, int dz, int dy, int dx, int xchunks,
                                                  int reach, int cap2, int32_t *__restrict__ fout,
                                                  int32_t *__restrict__ dist2, int32_t *__restrict__ nearest) {
  const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
  unsigned b = blockIdx.x;
  const int xc = (int)(b % (unsigned)xchunks);
  b /= (unsigned)xchunks;
  int z, y;
  if (AXIS == 1) {
    const unsigned groups = (unsigned)(dy + 3) >> 2;
    y = (int)(b % groups) * 4 + w;
    z = (int)(b / groups);
  } else {
    y = (int)(b % (unsigned)dy);
    z = (int)(b / (unsigned)dy) * 4 + w;
  }
  if (y >= dy || z >= dz) return;                           // wave-uniform
  const int xs = xc * 64 + lane;
  const int x = min(xs, dx - 1);                            // lanes past the row end repeat its last voxel, store none
  const int a = AXIS == 1 ? y : z, alen = AXIS == 1 ? dy : dz;
  const int64_t stride = AXIS == 1 ? (int64_t)dx : (int64_t)dy * dx;
  const int64_t self = ((int64_t)z * dy + y) * dx + x;
  const int32_t *col = fin + (self - a * stride);           // the voxel's column: col[a' * stride], a' in [0, alen)
  uint64_t best = edt_key(col[a * stride], z, y, x);
  const int last = min(reach, max(a, alen - 1 - a));        // the largest offset that is inside the axis and the reach
  for (int d = 1; d <= last; d += 4) {
    if (!__any((uint32_t)(d * d) <= (uint32_t)(best >> 32))) break;
    uint64_t k[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int lo = max(a - d - j, 0), hi = min(a + d + j, alen - 1);
      k[2 * j] = edt_key(col[lo * stride], z, y, x);
      k[2 * j + 1] = edt_key(col[hi * stride], z, y, x);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) best = min(best, k[j]);
  }
  if (xs >= dx) return;
  const uint32_t d2 = (uint32_t)(best >> 32);
  const int32_t f = (int32_t)(uint32_t)best;
  const bool none = best == NO_KEY || d2 > (uint32_t)cap2;
  if (LAST) {
    dist2[self] = none ? -1 : (int32_t)d2;
    nearest[self] = none ? -1 : (int32_t)((((int64_t)(f >> 20) * dy) + ((f >> 10) & 1023)) * dx + (f & 1023));
  } else {
    fout[self] = none ? -1 : f;
  }
}

__global__ __launch_bounds__(256) void k_edt_fill(const uint8_t *__restrict__ colors,
                                                  const int32_t *__restrict__ nearest, int64_t n,
                                                  uint8_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t s = nearest[i];
  uint8_t r = 0, g = 0, b = 0;
  if ((uint32_t)s < (uint32_t)n) {                          // -1, and anything that is no voxel of this volume
    const uint8_t *c = colors + (int64_t)s * 3;
    r = c[0], g = c[1], b = c[2];
  }
  uint8_t *o = out + i * 3;
  o[0] = r, o[1] = g, o[2] = b;
}

constexpr int64_t LIMIT = (int64_t)1 << 31;

// the largest d with d * d <= cap2
int edt_reach(int cap2) {
  int d = 0;
  while (d < EDT_MAX_DIM && (int64_t)(d + 1) * (d + 1) <= cap2) ++d;
  return d;
}

bool edt_dims_ok(int dz, int dy, int dx) {
  return dz >= 0 && dy >= 0 && dx >= 0 && dz <= EDT_MAX_DIM && dy <= EDT_MAX_DIM && dx <= EDT_MAX_DIM &&
         (int64_t)dz * dy * dx < LIMIT;
}

}  // namespace

SGNN_EXPORT int sgnn_edt_rows(const uint8_t *mask, int dz, int dy, int dx, int max_dist2, int32_t *feat,
                              sgnn_stream_t stream) {
  SGNN_CHECK_ARG(edt_dims_ok(dz, dy, dx));
  const int64_t rows = (int64_t)dz * dy;
  if (rows * dx == 0) return SGNN_OK;
  SGNN_CHECK_ARG(mask && feat);
  const int cap2 = max_dist2 < 0 ? INT32_MAX : max_dist2;
  SGNN_LAUNCH(k_edt_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, mask, rows, dy, dx, cap2,
              feat);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_edt_axis(const int32_t *feat_in, int dz, int dy, int dx, int axis, int max_dist2,
                              int32_t *feat_out, int32_t *dist2, int32_t *nearest, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(edt_dims_ok(dz, dy, dx));
  SGNN_CHECK_ARG(axis == 0 || axis == 1);
  SGNN_CHECK_ARG((dist2 != nullptr) == (nearest != nullptr));
  if ((int64_t)dz * dy * dx == 0) return SGNN_OK;
  const bool last = dist2 != nullptr;
  SGNN_CHECK_ARG(feat_in && (last || feat_out));
  SGNN_CHECK_ARG(feat_in != feat_out && feat_in != dist2 && feat_in != nearest);      // a pass reads its neighbours
  const int cap2 = max_dist2 < 0 ? INT32_MAX : max_dist2;
  const int reach = edt_reach(cap2);
  const int xchunks = (dx + 63) / 64;
  const int64_t blocks = axis == 1 ? (int64_t)xchunks * ((dy + 3) / 4) * dz : (int64_t)xchunks * dy * ((dz + 3) / 4);
  const dim3 grid((unsigned)blocks);             // <= the number of voxels < 2^31
  const hipStream_t s = (hipStream_t)stream;
  if (axis == 1) {
    if (last)
      SGNN_LAUNCH((k_edt_axis<1, true>), grid, dim3(256), 0, s, feat_in, dz, dy, dx, xchunks, reach, cap2, feat_out,
                  dist2, nearest);
    else
      SGNN_LAUNCH((k_edt_axis<1, false>), grid, dim3(256), 0, s, feat_in, dz, dy, dx, xchunks, reach, cap2, feat_out,
                  dist2, nearest);
  } else {
    if (last)
      SGNN_LAUNCH((k_edt_axis<0, true>), grid, dim3(256), 0, s, feat_in, dz, dy, dx, xchunks, reach, cap2, feat_out,
                  dist2, nearest);
    else
      SGNN_LAUNCH((k_edt_axis<0, false>), grid, dim3(256), 0, s, feat_in, dz, dy, dx, xchunks, reach, cap2, feat_out,
                  dist2, nearest);
  }
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_edt_fill(const uint8_t *colors, const int32_t *nearest, int64_t n, uint8_t *out,
                              sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && n < LIMIT);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(colors && nearest && out && colors != out);
  SGNN_LAUNCH(k_edt_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, colors, nearest, n,
              out);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
