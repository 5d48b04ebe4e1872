// Training chunks cut from a fused scan pair (sgnn_amd/chunks.py; rules in INTEGRATION.md "Training chunks"): the
// step between fusion.hip's volumes and the collated batch train.py consumes, without .sdfs files in between.
//
// Kernels (all streaming, HBM-bound; no floating-point atomics, so every result is exact and order-independent):
//   k_chunk_score         both fine volumes once -> per 8x8x8 brick {target voxels in the training band, input
//                         voxels a loader would keep}; a wave covers 8 bricks along x, a (z, y) row of 64 voxels per
//                         iteration, ballot + popcount per brick byte
//   k_chunk_window_sums   brick counts -> counts of every window of the stride grid (a wave per window)
//   k_chunk_flag          mask over B x crop voxels of the input volume: |sdf| <= keep and |sdf/vs| < truncation
//   k_chunk_emit_rows     kept voxels -> [z, y, x, b] int64 rows relative to the crop origin + sdf/vs features
//   k_chunk_crop          B windows of one pyramid level -> dense (B, 1, Z, Y, X) (sdf/f)/vs or -inf, and (level 0)
//                         the u8 known codes; one launch per level
// Compaction between flag and emit is sgnn_compact_mask (stable: crops in batch order, raster order inside a crop).
//
// flag and crop handle four x-consecutive voxels per thread: one 16-byte load where the source row is 16-byte
// aligned (volume x extent and window x origin multiples of 4: always so for the fine level of a volume whose x
// extent is a multiple of 4), four 4-byte loads otherwise (coarse levels); the fp32 rows go out as 16-byte stores.
// Voxels outside the volume are never read: the index is clamped to 0 and the value replaced, no branch per voxel.
//
// Built with -ffp-contract=off (Makefile): the fp32 expressions below are the ones of k_fuse_flag / k_fuse_known
// and of the file route (writer: sdf_f / f in metres, loader: / voxel size), one rounding each.
#include <math.h>
#include "common.h"

namespace {

constexpr int BRICK = 8;          // scoring brick edge; window origins, strides and extents are multiples of it

struct Vol {
  const float *sdf;
  int dx, dy, dz;
};

// four x-consecutive voxels (x0 .. x0+3, row y, slice z) of a volume, -inf (never observed) where the voxel is
// outside; returns bit i set when voxel i is inside
__device__ __forceinline__ unsigned load4(const Vol &v, int z, int y, int x0, float out[4]) {
  const float fill = -INFINITY;
  const bool row_in = z >= 0 && z < v.dz && y >= 0 && y < v.dy;
  const int64_t row = row_in ? ((int64_t)z * v.dy + y) * v.dx : 0;
  const bool vec = ((x0 | v.dx) & 3) == 0 && (reinterpret_cast<uintptr_t>(v.sdf) & 15) == 0;
  if (vec) {                                       // uniform over a crop: depends on the origin and the volume only
    const bool in = row_in && x0 >= 0 && x0 < v.dx;              // dx % 4 == 0: all four inside or none
    const float4 q = *reinterpret_cast<const float4 *>(v.sdf + (in ? row + x0 : 0));
    out[0] = in ? q.x : fill;
    out[1] = in ? q.y : fill;
    out[2] = in ? q.z : fill;
    out[3] = in ? q.w : fill;
    return in ? 15u : 0u;
  } else {
    unsigned inside = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int x = x0 + i;
      const bool in = row_in && x >= 0 && x < v.dx;
      const float s = v.sdf[in ? row + x : 0];
      out[i] = in ? s : fill;
      inside |= (unsigned)in << i;
    }
    return inside;
  }
}

// block = 4 waves = 4 brick rows (y) of one brick slice (z); wave = 8 bricks along x; lane = x within those 64 voxels
__global__ __launch_bounds__(256) void k_chunk_score(const float *__restrict__ tgt, const float *__restrict__ inp,
                                                    int dx, int dy, int dz, int nbx, int nby, float vs,
                                                    float truncation, float keep_abs, int32_t *__restrict__ bricks) {
  const int lane = threadIdx.x & 63;
  const int by = blockIdx.y * 4 + (int)(threadIdx.x >> 6), bz = blockIdx.z;
  if (by >= nby) return;                           // whole wave
  const int x = blockIdx.x * 64 + lane;
  const bool x_in = x < dx;
  int n_t = 0, n_i = 0;                            // lane b < 8: counts of brick blockIdx.x * 8 + b
  for (int k = 0; k < BRICK; ++k) {
    const int z = bz * BRICK + k;
#pragma unroll
    for (int j = 0; j < BRICK; ++j) {
      const int y = by * BRICK + j;
      const bool in = x_in && y < dy && z < dz;
      const int64_t v = in ? ((int64_t)z * dy + y) * dx + x : 0;
      const float t = tgt[v], s = inp[v];
      const bool ft = in && fabsf(__fdiv_rn(t, vs)) < truncation;
      const bool fi = in && fabsf(s) <= keep_abs && fabsf(__fdiv_rn(s, vs)) < truncation;
      const unsigned long long bt = __ballot(ft), bi = __ballot(fi);
      n_t += __popcll((bt >> (8 * (lane & 7))) & 0xFFull);
      n_i += __popcll((bi >> (8 * (lane & 7))) & 0xFFull);
    }
  }
  const int bx = blockIdx.x * 8 + lane;
  if (lane < 8 && bx < nbx) {
    const int64_t b = ((int64_t)bz * nby + by) * nbx + bx;
    reinterpret_cast<int2 *>(bricks)[b] = make_int2(n_t, n_i);
  }
}

struct Windows {
  int cz, cy, cx;      // window extent in bricks
  int sz, sy, sx;      // stride in bricks
  int nwz, nwy, nwx;   // windows per axis
};

// one wave per window: lanes stride over the window's bricks (those inside the brick grid), butterfly sum
__global__ __launch_bounds__(64) void k_chunk_window_sums(const int32_t *__restrict__ bricks, int nbx, int nby, int nbz,
                                                         Windows w, int32_t *__restrict__ table) {
  const int win = blockIdx.x;
  const int wx = win % w.nwx, wy = (win / w.nwx) % w.nwy, wz = win / (w.nwx * w.nwy);
  const int z0 = wz * w.sz, y0 = wy * w.sy, x0 = wx * w.sx;
  const int ez = max(min(w.cz, nbz - z0), 0), ey = max(min(w.cy, nby - y0), 0), ex = max(min(w.cx, nbx - x0), 0);
  const int n = ez * ey * ex;
  int n_t = 0, n_i = 0;
  for (int q = threadIdx.x; q < n; q += 64) {
    const int i = q % ex, j = (q / ex) % ey, k = q / (ex * ey);
    const int2 c = reinterpret_cast<const int2 *>(bricks)[((int64_t)(z0 + k) * nby + (y0 + j)) * nbx + (x0 + i)];
    n_t += c.x;
    n_i += c.y;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_t += __shfl_xor(n_t, off);
    n_i += __shfl_xor(n_i, off);
  }
  if (threadIdx.x == 0) reinterpret_cast<int2 *>(table)[win] = make_int2(n_t, n_i);
}

struct Crop {
  int nb, cz, cy, cx;  // crops and their extent in voxels of the level (cx % 4 == 0)
  int shift;           // origins are in fine voxels: level origin = origin >> shift
};

// thread t -> (b, z, y, x0) of its four voxels inside the crop, and the volume coordinates of the first
__device__ __forceinline__ void crop_site(const Crop &c, const int32_t *__restrict__ origins, int64_t t, int &b,
                                          int &z, int &y, int &x0, int &vz, int &vy, int &vx) {
  const int qx = c.cx >> 2;
  x0 = (int)(t % qx) << 2;
  const int64_t r = t / qx;
  y = (int)(r % c.cy);
  const int64_t r2 = r / c.cy;
  z = (int)(r2 % c.cz);
  b = (int)(r2 / c.cz);
  vz = (origins[3 * b] >> c.shift) + z;
  vy = (origins[3 * b + 1] >> c.shift) + y;
  vx = (origins[3 * b + 2] >> c.shift) + x0;
}

__global__ __launch_bounds__(256) void k_chunk_flag(Vol v, const int32_t *__restrict__ origins, Crop c, int64_t nq,
                                                   float keep_abs, float truncation, float vs,
                                                   uint32_t *__restrict__ mask4) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < nq; t += stride) {
    int b, z, y, x0, vz, vy, vx;
    crop_site(c, origins, t, b, z, y, x0, vz, vy, vx);
    float s[4];
    load4(v, vz, vy, vx, s);
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool keep = fabsf(s[i]) <= keep_abs && fabsf(__fdiv_rn(s[i], vs)) < truncation;
      m |= (uint32_t)keep << (8 * i);
    }
    mask4[t] = m;                                  // four u8 flags, x ascending (little endian)
  }
}

__global__ __launch_bounds__(256) void k_chunk_emit_rows(Vol v, const int32_t *__restrict__ origins, Crop c, float vs,
                                                        const int32_t *__restrict__ sel,
                                                        const int64_t *__restrict__ count,
                                                        int64_t *__restrict__ locs, float *__restrict__ feats) {
  const int64_t m = *count;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < m; q += stride) {
    const int64_t e = sel[q];                      // flagged, so inside the volume
    const int x = (int)(e % c.cx);
    const int64_t r = e / c.cx;
    const int y = (int)(r % c.cy);
    const int64_t r2 = r / c.cy;
    const int z = (int)(r2 % c.cz), b = (int)(r2 / c.cz);
    const int vz = origins[3 * b] + z, vy = origins[3 * b + 1] + y, vx = origins[3 * b + 2] + x;
    const bool in = vz >= 0 && vz < v.dz && vy >= 0 && vy < v.dy && vx >= 0 && vx < v.dx;
    const float s = v.sdf[in ? ((int64_t)vz * v.dy + vy) * v.dx + vx : 0];
    longlong2 *o = reinterpret_cast<longlong2 *>(locs + 4 * q);
    o[0] = make_longlong2((long long)z, (long long)y);
    o[1] = make_longlong2((long long)x, (long long)b);
    feats[q] = __fdiv_rn(s, vs);
  }
}

// out = |sdf| <= keep_abs ? (sdf / factor) / vs : -inf; known (level 0 only) = the .knw code, 255 outside the volume
__global__ __launch_bounds__(256) void k_chunk_crop(Vol v, const int32_t *__restrict__ origins, Crop c, int64_t nq,
                                                   float keep_abs, float factor, float vs, float *__restrict__ out,
                                                   uint8_t *__restrict__ known) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < nq; t += stride) {
    int b, z, y, x0, vz, vy, vx;
    crop_site(c, origins, t, b, z, y, x0, vz, vy, vx);
    float s[4], o[4];
    const unsigned inside = load4(v, vz, vy, vx, s);
    uint32_t kn = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[i] = fabsf(s[i]) <= keep_abs ? __fdiv_rn(__fdiv_rn(s[i], factor), vs) : -INFINITY;
      kn |= (uint32_t)((inside >> i) & 1u ? sgnn_known_code(s[i], vs) : 255) << (8 * i);
    }
    reinterpret_cast<float4 *>(out)[t] = make_float4(o[0], o[1], o[2], o[3]);
    if (known) reinterpret_cast<uint32_t *>(known)[t] = kn;
  }
}

bool crop_args_ok(int nb, int cz, int cy, int cx, int shift) {
  return nb >= 1 && cz >= 1 && cy >= 1 && cx >= 4 && (cx & 3) == 0 && shift >= 0 && shift <= 8 &&
         (int64_t)nb * cz * cy * cx < ((int64_t)1 << 31);
}

}  // namespace

SGNN_EXPORT int sgnn_chunk_score(const float *sdf_target, const float *sdf_input, int dx, int dy, int dz,
                                 float voxel_size, float truncation, float keep_abs, int cz, int cy, int cx, int sz,
                                 int sy, int sx, int nwz, int nwy, int nwx, int32_t *bricks, int32_t *table,
                                 sgnn_stream_t stream) {
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && dz >= 1 && dz <= 65535 * BRICK && voxel_size > 0.f);
  SGNN_CHECK_ARG(cz >= BRICK && cy >= BRICK && cx >= BRICK && sz >= BRICK && sy >= BRICK && sx >= BRICK);
  SGNN_CHECK_ARG((cz | cy | cx | sz | sy | sx) % BRICK == 0);
  SGNN_CHECK_ARG(nwz >= 1 && nwy >= 1 && nwx >= 1 && (int64_t)nwz * nwy * nwx < ((int64_t)1 << 31));
  SGNN_CHECK_ARG((int64_t)cz * cy * cx < ((int64_t)1 << 31));             // a window's count fits an int32
  SGNN_CHECK_ARG(sdf_target && sdf_input && bricks && table);
  SGNN_CHECK_ARG((reinterpret_cast<uintptr_t>(bricks) & 7) == 0 && (reinterpret_cast<uintptr_t>(table) & 7) == 0);
  const int nbx = (dx + BRICK - 1) / BRICK, nby = (dy + BRICK - 1) / BRICK, nbz = (dz + BRICK - 1) / BRICK;
  SGNN_CHECK_ARG((nby + 3) / 4 <= 65535);
  SGNN_LAUNCH(k_chunk_score, dim3((nbx + 7) / 8, (nby + 3) / 4, nbz), dim3(256), 0, (hipStream_t)stream, sdf_target,
              sdf_input, dx, dy, dz, nbx, nby, voxel_size, truncation, keep_abs, bricks);
  SGNN_CHECK_LAUNCH();
  const Windows w{cz / BRICK, cy / BRICK, cx / BRICK, sz / BRICK, sy / BRICK, sx / BRICK, nwz, nwy, nwx};
  SGNN_LAUNCH(k_chunk_window_sums, dim3(nwz * nwy * nwx), dim3(64), 0, (hipStream_t)stream, bricks, nbx, nby, nbz, w,
              table);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_chunk_flag(const float *sdf, int dx, int dy, int dz, const int32_t *origins, int nb, int cz,
                                int cy, int cx, float keep_abs, float truncation, float voxel_size, uint8_t *mask,
                                sgnn_stream_t stream) {
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && dz >= 1 && voxel_size > 0.f && crop_args_ok(nb, cz, cy, cx, 0));
  SGNN_CHECK_ARG(sdf && origins && mask && (reinterpret_cast<uintptr_t>(mask) & 3) == 0);
  const int64_t nq = (int64_t)nb * cz * cy * (cx / 4);
  SGNN_LAUNCH(k_chunk_flag, dim3(sgnn_grid_for(nq, 256, 8192)), dim3(256), 0, (hipStream_t)stream, Vol{sdf, dx, dy, dz},
              origins, Crop{nb, cz, cy, cx, 0}, nq, keep_abs, truncation, voxel_size,
              reinterpret_cast<uint32_t *>(mask));
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_chunk_emit_rows(const float *sdf, int dx, int dy, int dz, const int32_t *origins, int nb, int cz,
                                     int cy, int cx, float voxel_size, const int32_t *sel, const int64_t *count,
                                     int64_t n_max, int64_t *locs, float *feats, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && dz >= 1 && voxel_size > 0.f && n_max >= 0 && crop_args_ok(nb, cz, cy, cx, 0));
  if (n_max == 0) return SGNN_OK;
  SGNN_CHECK_ARG(sdf && origins && sel && count && locs && feats);
  SGNN_LAUNCH(k_chunk_emit_rows, dim3(sgnn_grid_for(n_max, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
              Vol{sdf, dx, dy, dz}, origins, Crop{nb, cz, cy, cx, 0}, voxel_size, sel, count, locs, feats);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_chunk_crop(const float *sdf, int dx, int dy, int dz, const int32_t *origins, int nb, int cz, int cy,
                                int cx, int shift, float keep_abs, float voxel_size, float *out, uint8_t *known,
                                sgnn_stream_t stream) {
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && dz >= 1 && voxel_size > 0.f && crop_args_ok(nb, cz, cy, cx, shift));
  SGNN_CHECK_ARG(sdf && origins && out && (reinterpret_cast<uintptr_t>(out) & 15) == 0);
  SGNN_CHECK_ARG((reinterpret_cast<uintptr_t>(known) & 3) == 0);
  const int64_t nq = (int64_t)nb * cz * cy * (cx / 4);
  SGNN_LAUNCH(k_chunk_crop, dim3(sgnn_grid_for(nq, 256, 8192)), dim3(256), 0, (hipStream_t)stream, Vol{sdf, dx, dy, dz},
              origins, Crop{nb, cz, cy, cx, shift}, nq, keep_abs, (float)(1 << shift), voxel_size, out, known);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
