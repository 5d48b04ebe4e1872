// The gravity-aligned room frame of a scan volume (sgnn_amd.upright): votes of the surface normals of a TSDF volume.
// The rules are listed in INTEGRATION.md section S; that text is the contract, and tests/upright_ref.py restates it
// independently in NumPy.  Every output is an integer count or a fixed-point integer sum, added with integer atomics:
// no launch detail and no atomic order shows in any bit of a result.
//
// All three kernels share one walk (up_walk): a workgroup of four waves takes four 64-voxel pieces of x rows at a
// time, so the centre loads of a wave are one coalesced 256-byte row piece; a lane whose centre fails |v| < surface
// (nearly all of them) leaves before the six neighbour loads, and the y and z neighbours of the few that stay come from
// the caches.  A surface voxel (rule S.1) is handed to the kernel's own functor.
//
// Kernels:
//   k_upright_histogram  rule S.2: the cube-map histogram of the normals, privatised per workgroup in LDS (24 KB at 32
//                        bins); only non-zero bins are flushed, one global atomic each.
//   k_upright_sums       rule S.4: grid = (blocks over the volume, records).  Eight int64 sums per lane, reduced per wave
//                        by shuffles and per block through LDS, then one 64-bit global atomic per block and slot.  The
//                        record is wave-uniform.
//   k_upright_heights    rule S.5: the two height histograms, privatised per workgroup in LDS (32 KB at 4096 bins).
//
// Built with -ffp-contract=off (Makefile): every product and sum is rounded on its own.
#include <math.h>
#include "common.h"
#include "geom.h"

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_GRID = 2048;
constexpr int HIST_MAX = 6 * 32 * 32;
constexpr float FIX = 1048576.0f;   // 2^20

struct UpVolume {
  const float *sdf;
  int dx, dy, dz;
  TsdfAffine w;   // world2grid
  float band, surface;
};

struct UpVoxel {
  int x, y, z;
  float v;      // the centre's sdf
  float m[3];   // M^T g
  float n[3];   // m / |m|
};

__device__ __forceinline__ float dot3(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// rule S.1 for every interior voxel; f(voxel) runs for the surface voxels only
template <typename F>
__device__ __forceinline__ void up_walk(const UpVolume &V, F f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pieces = (V.dx + 63) >> 6;
  const int64_t items = (int64_t)pieces * V.dy * V.dz;
  const int64_t sy = V.dx, sz = (int64_t)V.dx * V.dy;
  const float *M = V.w.m;
  for (int64_t it = (int64_t)blockIdx.x * 4 + wave; it < items; it += (int64_t)gridDim.x * 4) {
    const int piece = (int)(it % pieces);
    const int row = (int)(it / pieces);
    const int y = row % V.dy, z = row / V.dy;
    if (y < 1 || y > V.dy - 2 || z < 1 || z > V.dz - 2) continue;   // wave-uniform
    const int x = piece * 64 + lane;
    if (x < 1 || x > V.dx - 2) continue;
    const float *p = V.sdf + ((int64_t)z * sz + (int64_t)y * sy + x);
    const float v = p[0];
    if (!(fabsf(v) < V.surface) || !(fabsf(v) < V.band)) continue;   // a NaN or an infinity fails
    const float xm = p[-1], xp = p[1], ym = p[-sy], yp = p[sy], zm = p[-sz], zp = p[sz];
    if (!(fabsf(xm) < V.band && fabsf(xp) < V.band && fabsf(ym) < V.band && fabsf(yp) < V.band &&
          fabsf(zm) < V.band && fabsf(zp) < V.band))
      continue;
    const float gx = xp - xm, gy = yp - ym, gz = zp - zm;
    UpVoxel s;
    s.x = x, s.y = y, s.z = z, s.v = v;
#pragma unroll
    for (int k = 0; k < 3; ++k) s.m[k] = geom_linear_col(M, k, gx, gy, gz);
    if (!geom_unit<true>(s.m[0], s.m[1], s.m[2], s.n)) continue;
    f(s);
  }
}

__device__ __forceinline__ int up_cell(float a, int bins) {
  const int i = (int)(((a + 1.0f) * 0.5f) * (float)bins);
  return i < bins - 1 ? i : bins - 1;
}

__global__ __launch_bounds__(BLOCK) void k_upright_histogram(UpVolume V, int bins, int32_t *__restrict__ hist) {
  __shared__ int32_t local[HIST_MAX];
  const int nbin = 6 * bins * bins;
  for (int i = threadIdx.x; i < nbin; i += BLOCK) local[i] = 0;
  __syncthreads();
  up_walk(V, [&](const UpVoxel &s) {
    const float ax = fabsf(s.m[0]), ay = fabsf(s.m[1]), az = fabsf(s.m[2]);
    const int axis = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);   // ties: the lowest index
    const float major = axis == 0 ? s.m[0] : (axis == 1 ? s.m[1] : s.m[2]);
    const float ca = axis == 0 ? s.m[1] : (axis == 1 ? s.m[2] : s.m[0]);
    const float cb = axis == 0 ? s.m[2] : (axis == 1 ? s.m[0] : s.m[1]);
    const float am = fabsf(major);
    const int f = 2 * axis + (major < 0.f ? 1 : 0);
    const int iu = up_cell(__fdiv_rn(ca, am), bins), iv = up_cell(__fdiv_rn(cb, am), bins);
    atomicAdd(&local[(f * bins + iv) * bins + iu], 1);
  });
  __syncthreads();
  for (int i = threadIdx.x; i < nbin; i += BLOCK) {
    const int32_t c = local[i];
    if (c) atomicAdd(&hist[i], c);
  }
}

__global__ __launch_bounds__(BLOCK) void k_upright_sums(UpVolume V, const sgnn_upright_axis *__restrict__ records,
                                                       int64_t *__restrict__ out) {
  __shared__ long long part[4][8];
  const sgnn_upright_axis &R = records[blockIdx.y];
  bool rec_ok = fabsf(R.cos_cone) < INFINITY && fabsf(R.sin_wall) < INFINITY;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    rec_ok = rec_ok && fabsf(R.u[k]) < INFINITY && fabsf(R.e1[k]) < INFINITY && fabsf(R.e2[k]) < INFINITY;
  if (!rec_ok) return;   // a non-finite entry: an empty record (block-uniform)
  const float cos_cone = R.cos_cone, sin_wall = R.sin_wall;
  long long acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0;
  up_walk(V, [&](const UpVoxel &s) {
    const float t = dot3(s.n, R.u);
    const float at = fabsf(t);
    if (at >= cos_cone) {
      const float sg = t > 0.f ? 1.0f : (t < 0.f ? -1.0f : 0.0f);
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[k] += llrintf((sg * s.n[k]) * FIX);   // round half to even
      acc[3] += t > 0.f ? 1 : 0;
      acc[4] += t < 0.f ? 1 : 0;
    }
    if (at <= sin_wall) {
      const float a = dot3(s.n, R.e1), b = dot3(s.n, R.e2);
      const float r2 = a * a + b * b;
      if (r2 > 0.f) {
        const float r = (float)sqrt((double)r2);
        const float c = __fdiv_rn(a, r), d = __fdiv_rn(b, r);
        const float c2 = c * c - d * d, s2 = 2.0f * (c * d);
        const float c4 = c2 * c2 - s2 * s2, s4 = 2.0f * (s2 * c2);
        acc[5] += llrintf(c4 * FIX);
        acc[6] += llrintf(s4 * FIX);
        acc[7] += 1;
      }
    }
  });
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    long long v = acc[k];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) part[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const long long v = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
    if (v) atomicAdd((unsigned long long *)(out + (int64_t)blockIdx.y * 8 + threadIdx.x), (unsigned long long)v);
  }
}

__global__ __launch_bounds__(BLOCK) void k_upright_heights(UpVolume V, TsdfAffine g2w, float ux, float uy, float uz,
                                                          float cos_cone, float h0, float bin, int nbins,
                                                          int32_t *__restrict__ hist) {
  __shared__ int32_t local[2 * SGNN_UPRIGHT_MAX_HEIGHT_BINS];
  for (int i = threadIdx.x; i < 2 * nbins; i += BLOCK) local[i] = 0;
  __syncthreads();
  const float u[3] = {ux, uy, uz};
  up_walk(V, [&](const UpVoxel &s) {
    const float t = dot3(s.n, u);
    const int row = t >= cos_cone ? 0 : (t <= -cos_cone ? 1 : -1);
    if (row < 0) return;
    float p[3], q[3];
    tsdf_affine(g2w.m, (float)s.x, (float)s.y, (float)s.z, p);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = p[k] - s.v * s.n[k];
    const float kf = floorf(__fdiv_rn(dot3(q, u) - h0, bin));
    if (!(kf >= 0.f && kf < (float)nbins)) return;   // a NaN fails
    atomicAdd(&local[row * nbins + (int)kf], 1);
  });
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * nbins; i += BLOCK) {
    const int32_t c = local[i];
    if (c) atomicAdd(&hist[i], c);
  }
}

// 0: bad arguments; 1: nothing to do (a dimension below 3 has no interior voxel); 2: launch with `grid` blocks
int up_volume_arg(const float *sdf, int dx, int dy, int dz, const float *world2grid, float band, float surface,
                  UpVolume &V, int &grid) {
  if (!(dx >= 1 && dy >= 1 && dz >= 1 && (int64_t)dx * dy * dz < ((int64_t)1 << 31))) return 0;
  if (!(band > 0.f && surface > 0.f) || !world2grid) return 0;   // a NaN fails
  V.sdf = sdf, V.dx = dx, V.dy = dy, V.dz = dz, V.band = band, V.surface = surface;
  if (!tsdf_affine_arg(world2grid, V.w)) return 0;
  if (dx < 3 || dy < 3 || dz < 3) return 1;
  if (!sdf) return 0;
  const int64_t items = (int64_t)((dx + 63) >> 6) * dy * dz;
  grid = sgnn_grid_for(items, 4, MAX_GRID);
  return 2;
}

}  // namespace

SGNN_EXPORT int sgnn_upright_histogram(const float *sdf, int dx, int dy, int dz, const float *world2grid, float band,
                                       float surface, int bins, int32_t *hist, sgnn_stream_t stream) {
  UpVolume V;
  int grid = 0;
  const int go = up_volume_arg(sdf, dx, dy, dz, world2grid, band, surface, V, grid);
  SGNN_CHECK_ARG(go != 0 && (bins == 8 || bins == 16 || bins == 32));
  if (go == 1) return SGNN_OK;
  SGNN_CHECK_ARG(hist);
  SGNN_LAUNCH(k_upright_histogram, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, V, bins, hist);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_upright_sums(const float *sdf, int dx, int dy, int dz, const float *world2grid, float band,
                                  float surface, const sgnn_upright_axis *records, int nrecords, int64_t *out,
                                  sgnn_stream_t stream) {
  UpVolume V;
  int grid = 0;
  const int go = up_volume_arg(sdf, dx, dy, dz, world2grid, band, surface, V, grid);
  SGNN_CHECK_ARG(go != 0 && nrecords >= 0 && nrecords <= 65535);
  if (go == 1 || nrecords == 0) return SGNN_OK;
  SGNN_CHECK_ARG(records && out);
  SGNN_LAUNCH(k_upright_sums, dim3(grid, nrecords), dim3(BLOCK), 0, (hipStream_t)stream, V, records, out);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_upright_heights(const float *sdf, int dx, int dy, int dz, const float *world2grid,
                                     const float *grid2world, float band, float surface, const float *up,
                                     float cos_cone, float h0, float bin, int nbins, int32_t *hist,
                                     sgnn_stream_t stream) {
  UpVolume V;
  int grid = 0;
  const int go = up_volume_arg(sdf, dx, dy, dz, world2grid, band, surface, V, grid);
  SGNN_CHECK_ARG(go != 0 && nbins >= 1 && nbins <= SGNN_UPRIGHT_MAX_HEIGHT_BINS);
  TsdfAffine g2w;
  SGNN_CHECK_ARG(grid2world && tsdf_affine_arg(grid2world, g2w) && up);
  SGNN_CHECK_ARG(isfinite(up[0]) && isfinite(up[1]) && isfinite(up[2]) && cos_cone > 0.f && isfinite(cos_cone) && isfinite(h0) &&
                 bin > 0.f && isfinite(bin));
  if (go == 1) return SGNN_OK;
  SGNN_CHECK_ARG(hist);
  SGNN_LAUNCH(k_upright_heights, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, V, g2w, up[0], up[1], up[2], cos_cone,
              h0, bin, nbins, hist);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
