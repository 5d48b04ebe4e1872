// The camera and the sampled dense volume of the frame and pose tools, each expression written once so that the
// restatements in tests/*_ref.py hold every tool to the same bits; tsdf.h (the per-voxel TSDF state) includes it.
// No kernels here.  Every includer is built with -ffp-contract=off: each product and sum below is rounded on its own.
#pragma once
#include <math.h>
#include "common.h"

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }   // false for a NaN

// ---- affine maps: rows 0..2 of a 4x4, row-major --------------------------------------------------------------------
struct TsdfAffine { float m[12]; };

// ((m0 x + m1 y) + m2 z) + m3 of row r: the order of fusion._affine
__device__ __forceinline__ float tsdf_affine_row(const float *m, int r, float x, float y, float z) {
  return ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
}

__device__ __forceinline__ void tsdf_affine(const float *m, float x, float y, float z, float (&out)[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) out[r] = tsdf_affine_row(m, r, x, y, z);
}

// 0: an entry is not finite
static inline int tsdf_affine_arg(const float *host12, TsdfAffine &a) {
  for (int c = 0; c < 12; ++c) {
    if (!isfinite(host12[c])) return 0;
    a.m[c] = host12[c];
  }
  return 1;
}

// the linear part of such a map by rows, (m0 a + m1 b) + m2 c, and its transpose for a covector, (m0 a + m4 b) + m8 c
__device__ __forceinline__ float geom_linear_row(const float *m, int r, float a, float b, float c) {
  return (m[4 * r] * a + m[4 * r + 1] * b) + m[4 * r + 2] * c;
}
__device__ __forceinline__ float geom_linear_col(const float *m, int k, float a, float b, float c) {
  return (m[k] * a + m[4 + k] * b) + m[8 + k] * c;
}

// ---- the pinhole; intr = fx, fy, cx, cy as the frame records pack them; axis 0: x, 1: y ------------------------------
__device__ __forceinline__ float geom_unproject(const float *intr, int axis, float p) {   // pixel -> camera at z = 1
  return __fdiv_rn(p - intr[2 + axis], intr[axis]);
}
__device__ __forceinline__ float geom_project(const float *intr, int axis, float x, float z) {   // camera -> pixel
  return __fdiv_rn(x * intr[axis], z) + intr[2 + axis];
}

// ---- the unit vector: the correctly rounded length (the fp32 root is not), then three divisions.  False, n untouched,
// where the length is 0, infinite or NaN; SQUARE gates on the squared length before the root, as upright's rule S.1 does.
template <bool SQUARE = false>
__device__ __forceinline__ bool geom_unit(float x, float y, float z, float (&n)[3]) {
  const float len2 = (x * x + y * y) + z * z;
  if (SQUARE && !(len2 > 0.f && len2 < INFINITY)) return false;
  const float len = (float)sqrt((double)len2);
  if (!SQUARE && !(len > 0.f && len < INFINITY)) return false;
  n[0] = __fdiv_rn(x, len), n[1] = __fdiv_rn(y, len), n[2] = __fdiv_rn(z, len);
  return true;
}

// ---- the cell of grid position g in a dense (dz, dy, dx) volume.  regrid.hip's rule 5 is NOT this cell and stays on its
// own: there an axis with a == 0 contributes one index and a zero-weight corner is never read.
struct GeomCell { int64_t base; float a[3]; };   // voxel index of corner f = floor(g); g - f (x, y, z)
// false, and c untouched, where 0 <= f <= d - 2 fails on an axis (a NaN fails)
__device__ __forceinline__ bool geom_cell(int dx, int dy, int dz, float gx, float gy, float gz, GeomCell &c) {
  const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
  if (!(fx >= 0.f && fx <= (float)(dx - 2) && fy >= 0.f && fy <= (float)(dy - 2) && fz >= 0.f &&
        fz <= (float)(dz - 2)))
    return false;
  c.base = ((int64_t)(int)fz * dy + (int)fy) * dx + (int)fx;
  c.a[0] = gx - fx, c.a[1] = gy - fy, c.a[2] = gz - fz;
  return true;
}

// offset of corner i from corner f in voxels (x fastest, then y, then z); the 8 corners at p, `stride` elements per voxel
__device__ __forceinline__ int64_t geom_corner(int dx, int dy, int i) {
  return (int64_t)(i >> 2) * dx * dy + (int64_t)((i >> 1) & 1) * dx + (i & 1);
}
template <typename T>
__device__ __forceinline__ void geom_gather(const T *p, int dx, int dy, T (&c)[8], int stride = 1) {
#pragma unroll
  for (int i = 0; i < 8; ++i) c[i] = p[geom_corner(dx, dy, i) * stride];
}

// the axis weights {1 - a, a} and the corner weight (wz * wy) * wx
struct GeomWeights {
  float x[2], y[2], z[2];
  __device__ __forceinline__ GeomWeights(const float (&a)[3])
      : x{1.0f - a[0], a[0]}, y{1.0f - a[1], a[1]}, z{1.0f - a[2], a[2]} {}
  __device__ __forceinline__ float corner(int i) const { return (z[i >> 2] * y[(i >> 1) & 1]) * x[i & 1]; }
};
