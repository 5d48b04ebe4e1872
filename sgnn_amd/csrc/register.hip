// Point sets registered against a TSDF volume (sgnn_amd.register): point-to-SDF Gauss-Newton.  The destination volume
// is already a distance field, so a source point needs no nearest-neighbour search: its residual is the trilinearly
// interpolated sdf at its transformed position and its Jacobian the gradient of the same interpolant.  The rules are
// listed in INTEGRATION.md section R; that text is the contract, and tests/register_ref.py restates it independently
// in NumPy.
//
// Kernels:
//   k_register_system  grid = (blocks over the points, records).  A lane walks points with a grid stride: one 8-corner
//                      gather per point (rules 2-4), the gates (rule 5), the row of rule 6, and the 28 sums of rule 7 as
//                      fp64 accumulators with its point count.  The record is wave-uniform and arrives by scalar
//                      loads.  Points are unordered, so the gathers are not coalesced; no LDS staging and no sort.  A
//                      lane without an association adds zeros.  Reduction: csrc/gn_system.h.
//   k_gn_finish        one block per record adds the partials in index order (csrc/gn_system.h).
//
// Built with -ffp-contract=off (Makefile): every product and sum is rounded on its own.
#include <math.h>
#include "common.h"
#include "gn_system.h"
#include "geom.h"

namespace {

constexpr int BLOCK = GN_BLOCK;

__device__ __forceinline__ float lerp(float p, float q, float a) { return p + a * (q - p); }

__global__ __launch_bounds__(BLOCK) void k_register_system(const float *__restrict__ points, int npts,
                                                          const float *__restrict__ sdf, int dx, int dy, int dz,
                                                          const sgnn_register_pair *__restrict__ pairs, float band,
                                                          float max_dist, float min_grad2, double *__restrict__ ws,
                                                          float *__restrict__ residual, int32_t *__restrict__ cell) {
  __shared__ double part[4][GN_ENTRIES];
  const int pair = (int)blockIdx.y;
  const sgnn_register_pair &P = pairs[pair];
  const float *T = P.t, *W = P.w;
  const bool rec_ok = T[0] == T[0];                 // non-finite record (the host stores NaN): an empty system
  const int64_t sy = dx, sz = (int64_t)dx * dy;
  const int64_t out0 = (int64_t)pair * npts;
  double acc[GN_NSUM];
#pragma unroll
  for (int k = 0; k < GN_NSUM; ++k) acc[k] = 0.0;
  int count = 0;
  for (int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x; i < npts; i += (int)gridDim.x * BLOCK) {
    // rule 2
    const float px = points[(int64_t)i * 3 + 0], py = points[(int64_t)i * 3 + 1], pz = points[(int64_t)i * 3 + 2];
    float q[3], g[3];
    tsdf_affine(T, px, py, pz, q);
    tsdf_affine(W, q[0], q[1], q[2], g);
    bool ok = rec_ok && finite_f(px) && finite_f(py) && finite_f(pz) && finite_f(q[0]) && finite_f(q[1]) &&
              finite_f(q[2]) && finite_f(g[0]) && finite_f(g[1]) && finite_f(g[2]);
    // rule 3: the cell and its 8 corners; a lane without a cell reads cell 0, which every volume has (dims >= 2).
    // Written out, not on geom.h's cell helpers: their array form compiled worse here, and speed wins over sharing.
    const float fx = floorf(g[0]), fy = floorf(g[1]), fz = floorf(g[2]);
    ok = ok && fx >= 0.f && fx <= (float)(dx - 2) && fy >= 0.f && fy <= (float)(dy - 2) && fz >= 0.f &&
         fz <= (float)(dz - 2);
    const int lin = ok ? ((int)fz * dy + (int)fy) * dx + (int)fx : 0;
    const float *p = sdf + lin;
    const float c000 = p[0], c001 = p[1], c010 = p[sy], c011 = p[sy + 1];
    const float c100 = p[sz], c101 = p[sz + 1], c110 = p[sz + sy], c111 = p[sz + sy + 1];
    ok = ok && fabsf(c000) < band && fabsf(c001) < band && fabsf(c010) < band && fabsf(c011) < band &&
         fabsf(c100) < band && fabsf(c101) < band && fabsf(c110) < band && fabsf(c111) < band;   // NaN, inf: false
    const float ax = g[0] - fx, ay = g[1] - fy, az = g[2] - fz;
    const float v = lerp(lerp(lerp(c000, c001, ax), lerp(c010, c011, ax), ay),
                         lerp(lerp(c100, c101, ax), lerp(c110, c111, ax), ay), az);
    // rule 4: the gradient of that interpolant, per voxel, and the world-space covector
    const float gx = lerp(lerp(c001 - c000, c011 - c010, ay), lerp(c101 - c100, c111 - c110, ay), az);
    const float gy = lerp(lerp(c010 - c000, c011 - c001, ax), lerp(c110 - c100, c111 - c101, ax), az);
    const float gz = lerp(lerp(c100 - c000, c101 - c001, ax), lerp(c110 - c010, c111 - c011, ax), ay);
    const float nx = geom_linear_col(W, 0, gx, gy, gz), ny = geom_linear_col(W, 1, gx, gy, gz);
    const float nz = geom_linear_col(W, 2, gx, gy, gz);
    // rule 5
    const float len2 = (nx * nx + ny * ny) + nz * nz;
    ok = ok && fabsf(v) <= max_dist && finite_f(len2) && len2 >= min_grad2;
    // rules 6 and 8
    if (residual) residual[out0 + i] = ok ? v : NAN;
    if (cell) cell[out0 + i] = ok ? lin : -1;
    float J[7];
    J[0] = ok ? q[1] * nz - q[2] * ny : 0.f;
    J[1] = ok ? q[2] * nx - q[0] * nz : 0.f;
    J[2] = ok ? q[0] * ny - q[1] * nx : 0.f;
    J[3] = ok ? nx : 0.f;
    J[4] = ok ? ny : 0.f;
    J[5] = ok ? nz : 0.f;
    J[6] = ok ? v : 0.f;
    gn_accumulate(acc, J);                          // rule 7: exact products, fp64 sums
    count += ok ? 1 : 0;
  }
  gn_block_reduce(acc, count, part, ws + ((int64_t)pair * gridDim.x + blockIdx.x) * GN_ENTRIES);
}

}  // namespace

SGNN_EXPORT int sgnn_register_system(const float *points, int npoints, const float *sdf, int dx, int dy, int dz,
                                     const sgnn_register_pair *pairs, int npairs, float band, float max_dist,
                                     float min_grad2, double *out, float *residual, int32_t *cell, void *ws,
                                     int64_t ws_bytes, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(npoints >= 0 && npairs >= 0 && npairs <= 65535);
  SGNN_CHECK_ARG((int64_t)npoints < ((int64_t)1 << 31) - (int64_t)SGNN_REGISTER_MAX_BLOCKS * BLOCK);   // the stride loop's index
  SGNN_CHECK_ARG(dx >= 2 && dy >= 2 && dz >= 2 && (int64_t)dx * dy * dz < ((int64_t)1 << 31));       // the cell is an int32
  SGNN_CHECK_ARG(band > 0.f && max_dist > 0.f && min_grad2 >= 0.f);                                  // a NaN fails
  if (npoints == 0 || npairs == 0) return SGNN_OK;
  SGNN_CHECK_ARG(points && sdf && pairs && out && ws);
  hipStream_t s = (hipStream_t)stream;
  return gn_launch(npoints, SGNN_REGISTER_MAX_BLOCKS, npairs, ws, ws_bytes, out, s, [&](int nblk) {
    SGNN_LAUNCH(k_register_system, dim3(nblk, npairs), dim3(BLOCK), 0, s, points, npoints, sdf, dx, dy, dz, pairs, band,
                max_dist, min_grad2, (double *)ws, residual, cell);
  });
}
