// Point-cloud neighbourhoods: a uniform grid over a point set, exact k nearest neighbours, radius counts and lists,
// PCA normals, mean neighbour distances and voxel down-sampling (include/sgnn_hip.h, "Point-cloud neighbourhoods";
// rules in INTEGRATION.md section Z, restated on the host without a grid in tests/cloud_ref.py).
//
// This file is compiled with -ffp-contract=off.  Distances are fp32 (dx*dx + dy*dy) + dz*dz, each operation rounded
// once; normals, means and voxel sums are fp64 + - * / and the correctly rounded root in the order section Z writes
// down: the NumPy restatement gives the same bits.  No floating-point atomics; every sum is taken in list order.
//
//   k_cloud_keys          one thread per point: (cell << 32 | index), cell 2^31 - 1 for a non-finite row
//   k_cloud_pack          one thread per sorted key: the point as (x, y, z, index) in cell order, and the cell starts
//   k_cloud_knn<K, SELF>  one lane per query, queries in cell order: rings of cells outward, the K best (d2, index)
//                         keys in registers (an unrolled compare-exchange chain, no run-time index: no scratch)
//   k_cloud_radius<FILL>  the same walk with a fixed bound: a count, or (query << 32 | index) keys behind a scan
//   k_cloud_normals       one lane per point: fp64 covariance of its kNN row, five cyclic Jacobi sweeps (rule C.3)
//   k_cloud_mean_dist     one lane per point: fp64 mean of the fp32 roots of its kNN row (rule C.4)
//   k_cloud_voxel_keys, k_cloud_run_flags, k_cloud_voxel_reduce      rule C.5
//
// The walk is bound by the latency of its dependent loads (cell start, then points): a cell's points are 16-byte
// records, contiguous, and a whole x-range of cells of a ring's face is one range; four records are in flight.
#include "common.h"

namespace {

constexpr int64_t LIMIT = (int64_t)1 << 31;
constexpr uint32_t CELL_NONE = 0x7FFFFFFFu;                // the cell field of a non-finite row: sorts behind every cell
constexpr uint64_t SLOT_EMPTY = ~0ull;                     // above every (d2, index) key: the d2 field is not a distance
constexpr uint64_t VKEY_NONE = 0x7FFFFFFFFFFFFFFFull;      // voxel key of a row that has no voxel
constexpr int MAX_AXIS = 1024;                             // cells per axis (rule C.2 rests on it)
constexpr int VOXEL_LIMIT = 1 << 20;
constexpr int LONG_RUN = 128;                              // voxel runs above this are loaded by the whole wave

struct Grid {
  float lox, loy, loz, cell;
  int nx, ny, nz;
};

__device__ __forceinline__ bool cloud_finite(float x) { return fabsf(x) < __builtin_inff(); }      // false for a NaN

// Cell of a finite coordinate along one axis, clamped to the grid (rule C.2): floor((p - lo) / cell) in fp32.
__device__ __forceinline__ int cloud_bin(float p, float lo, float cell, int n) {
  const float t = floorf(__fdiv_rn(p - lo, cell));
  return (int)fminf(fmaxf(t, 0.f), (float)(n - 1));
}

__global__ __launch_bounds__(256) void k_cloud_keys(const float *__restrict__ pts, int64_t n, Grid g,
                                                   uint64_t *__restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
  uint32_t cell = CELL_NONE;
  if (cloud_finite(x) && cloud_finite(y) && cloud_finite(z))
    cell = (uint32_t)((cloud_bin(z, g.loz, g.cell, g.nz) * g.ny + cloud_bin(y, g.loy, g.cell, g.ny)) * g.nx +
                      cloud_bin(x, g.lox, g.cell, g.nx));
  keys[i] = (uint64_t)cell << 32 | (uint64_t)(uint32_t)i;
}

// Thread j < nfin writes record j; thread j <= nfin writes start[c] = j for every cell c behind the cell of record
// j - 1 up to the cell of record j (ncell for j = nfin): every entry of start (ncell + 1) is written exactly once.
__global__ __launch_bounds__(256) void k_cloud_pack(const float *__restrict__ pts, int64_t n,
                                                   const uint64_t *__restrict__ keys, int64_t nfin, int64_t ncell,
                                                   float4 *__restrict__ packed, int32_t *__restrict__ start) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j > nfin) return;
  int64_t c1 = ncell;
  if (j < nfin) {
    const uint64_t key = keys[j];
    const int64_t i = (int64_t)(key & 0xFFFFFFFFu);
    c1 = (int64_t)(key >> 32);
    if (i >= n || c1 >= ncell) return;      // never for keys of k_cloud_keys
    packed[j] = make_float4(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], __int_as_float((int)i));
  }
  int64_t c0 = j == 0 ? -1 : (int64_t)(keys[j - 1] >> 32);
  if (c0 >= ncell) c0 = ncell - 1;
  for (int64_t c = c0 + 1; c <= c1; ++c) start[c] = (int32_t)j;
}

// The walk of rule C.2: rings of cells of Chebyshev distance r = 0, 1, .. round the query's clamped cell, every cell of
// the grid at most once; f.take(d2, index) for every point of a visited cell, f.done(bound2) after every ring, where
// no unvisited point has d2 below bound2.
template <class F>
__device__ __forceinline__ void cloud_walk(const Grid g, const float4 *__restrict__ pts,
                                           const int32_t *__restrict__ start, float qx, float qy, float qz, F &f) {
  const int cx = cloud_bin(qx, g.lox, g.cell, g.nx), cy = cloud_bin(qy, g.loy, g.cell, g.ny),
            cz = cloud_bin(qz, g.loz, g.cell, g.nz);
  const int rmax = max(max(max(cx, g.nx - 1 - cx), max(cy, g.ny - 1 - cy)), max(cz, g.nz - 1 - cz));
  for (int r = 0; r <= rmax; ++r) {
    const int z0 = max(cz - r, 0), z1 = min(cz + r, g.nz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.ny - 1);
    for (int z = z0; z <= z1; ++z) {
      const bool zface = z == cz - r || z == cz + r;
      for (int y = y0; y <= y1; ++y) {
        const int row = (z * g.ny + y) * g.nx;
        // on a face of the ring the whole x-range, one contiguous range of points; else the two ends of the row
        const bool face = zface || y == cy - r || y == cy + r;
        for (int side = 0; side < 2; ++side) {
          int c0 = side ? cx + r : cx - r, c1 = c0;
          if (face) c0 = max(cx - r, 0), c1 = min(cx + r, g.nx - 1);
          if (side ? (face || c0 >= g.nx) : c0 < 0) continue;
          const int a = start[row + c0], b = start[row + c1 + 1];
          for (int j = a; j < b; j += 4) {
            float4 p[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) p[u] = pts[min(j + u, b - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              if (j + u >= b) continue;
              const float dx = qx - p[u].x, dy = qy - p[u].y, dz = qz - p[u].z;
              f.take((dx * dx + dy * dy) + dz * dz, __float_as_int(p[u].w));
            }
          }
        }
      }
    }
    // a point of an unvisited cell is more than cell * (r - 2^-11) away along one axis (section Z, C.2); the factor
    // 1 - 2^-9 keeps the fp32 product below that, and fp32 rounding is monotonic, so its d2 is at least bound2
    const float bound = (g.cell * (float)r) * 0.998046875f;
    if (f.done(bound * bound)) break;
  }
}

// The K best keys (bits(d2) << 32 | index) as K named members, worst first: Best<K>.head is the K-th best.  Every
// access is a member access resolved at compile time, so the list stays in registers (a per-lane array indexed in a
// loop is left in scratch above 8 entries).
template <int K>
struct Best {
  uint64_t head;
  Best<K - 1> tail;
  __device__ __forceinline__ void clear() { head = SLOT_EMPTY, tail.clear(); }
  __device__ __forceinline__ void insert(uint64_t c) {      // one step of the compare-exchange chain: c < head on entry
    const uint64_t hi = tail.head > c ? tail.head : c;
    head = head < hi ? head : hi;
    tail.insert(c);
  }
  __device__ __forceinline__ uint64_t at(int i) const { return i == K - 1 ? head : tail.at(i); }
  __device__ __forceinline__ void store(int64_t row, int k, int32_t *__restrict__ idx, float *__restrict__ d2) const {
    if (K - 1 < k) {
      idx[row * k + K - 1] = head == SLOT_EMPTY ? -1 : (int32_t)(uint32_t)(head & 0xFFFFFFFFu);
      d2[row * k + K - 1] = head == SLOT_EMPTY ? __builtin_inff() : __uint_as_float((uint32_t)(head >> 32));
    }
    tail.store(row, k, idx, d2);
  }
};

template <>
struct Best<1> {
  uint64_t head;
  __device__ __forceinline__ void clear() { head = SLOT_EMPTY; }
  __device__ __forceinline__ void insert(uint64_t c) { head = head < c ? head : c; }
  __device__ __forceinline__ uint64_t at(int) const { return head; }
  __device__ __forceinline__ void store(int64_t row, int k, int32_t *__restrict__ idx, float *__restrict__ d2) const {
    idx[row * k] = head == SLOT_EMPTY ? -1 : (int32_t)(uint32_t)(head & 0xFFFFFFFFu);
    d2[row * k] = head == SLOT_EMPTY ? __builtin_inff() : __uint_as_float((uint32_t)(head >> 32));
  }
};

template <int K>
struct KnnList {
  Best<K> best;
  float limit2;
  int self, k;
  __device__ __forceinline__ void take(float d2, int idx) {
    if (idx == self || !(d2 <= limit2)) return;
    const uint64_t c = (uint64_t)__float_as_uint(d2) << 32 | (uint64_t)(uint32_t)idx;
    if (c < best.head) best.insert(c);
  }
  __device__ __forceinline__ bool done(float bound2) const {
    const uint64_t kth = best.at(k - 1);
    return bound2 > limit2 || (kth != SLOT_EMPTY && __uint_as_float((uint32_t)(kth >> 32)) < bound2);
  }
};

// SELF: the queries are the indexed points themselves (record j), each without its own row.  Otherwise qkeys are the
// sorted keys of k_cloud_keys over the queries; rows go to the query's own place.
template <int K, bool SELF>
__global__ __launch_bounds__(256) void k_cloud_knn(Grid g, const float4 *__restrict__ pts,
                                                  const int32_t *__restrict__ start,
                                                  const float *__restrict__ queries,
                                                  const uint64_t *__restrict__ qkeys, int64_t nq, int64_t nrows, int k,
                                                  float limit2, int32_t *__restrict__ idx_out,
                                                  float *__restrict__ d2_out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nq) return;
  KnnList<K> list;
  list.best.clear();
  list.limit2 = limit2, list.k = k, list.self = -1;
  int64_t row;
  bool walk = true;
  float qx, qy, qz;
  if (SELF) {
    const float4 p = pts[j];
    qx = p.x, qy = p.y, qz = p.z;
    row = list.self = __float_as_int(p.w);
  } else {
    const uint64_t key = qkeys[j];
    row = (int64_t)(key & 0xFFFFFFFFu);
    walk = (uint32_t)(key >> 32) != CELL_NONE;
    if (row >= nrows) return;      // never for keys of k_cloud_keys
    qx = queries[3 * row], qy = queries[3 * row + 1], qz = queries[3 * row + 2];
  }
  if (row < 0 || row >= nrows) return;
  if (walk) cloud_walk(g, pts, start, qx, qy, qz, list);
  list.best.store(row, k, idx_out, d2_out);
}

struct RadiusList {
  float limit2;
  int64_t n, cap, row;
  uint64_t *out;
  __device__ __forceinline__ void take(float d2, int idx) {
    if (!(d2 <= limit2)) return;
    if (out && n < cap) out[n] = (uint64_t)row << 32 | (uint64_t)(uint32_t)idx;
    ++n;
  }
  __device__ __forceinline__ bool done(float bound2) const { return bound2 > limit2; }
};

template <bool FILL>
__global__ __launch_bounds__(256) void k_cloud_radius(Grid g, const float4 *__restrict__ pts,
                                                     const int32_t *__restrict__ start,
                                                     const float *__restrict__ queries,
                                                     const uint64_t *__restrict__ qkeys, int64_t nq, float limit2,
                                                     int32_t *__restrict__ count, const int64_t *__restrict__ qstart,
                                                     uint64_t *__restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nq) return;
  const uint64_t key = qkeys[j];
  const int64_t row = (int64_t)(key & 0xFFFFFFFFu);
  if (row >= nq) return;      // never for keys of k_cloud_keys
  RadiusList list = {limit2, 0, 0, row, nullptr};
  if (FILL) {
    list.out = out + qstart[row];
    list.cap = qstart[row + 1] - qstart[row];
  }
  if ((uint32_t)(key >> 32) != CELL_NONE)
    cloud_walk(g, pts, start, queries[3 * row], queries[3 * row + 1], queries[3 * row + 2], list);
  if (!FILL) count[row] = (int32_t)list.n;
}

// One Jacobi rotation of rule C.3 on the pair (p, q) with r the third index; v.p / v.q are the two columns of V.
__device__ __forceinline__ void cloud_rotate(double &app, double &aqq, double &apq, double &arp, double &arq,
                                             double (&vp)[3], double (&vq)[3]) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double a = vp[i], b = vq[i];
    vp[i] = c * a - s * b;
    vq[i] = s * a + c * b;
  }
}

// toward_mode 0: none, 1: one viewpoint (3 floats), 2: one per point (n, 3).
__global__ __launch_bounds__(256) void k_cloud_normals(const float *__restrict__ pts, int64_t n,
                                                      const int32_t *__restrict__ nbr, int k,
                                                      const float *__restrict__ toward, int toward_mode,
                                                      float *__restrict__ normal, float *__restrict__ variation,
                                                      uint8_t *__restrict__ valid) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int kk = 0;
  while (kk < k && (uint32_t)nbr[i * k + kk] < (uint32_t)n) ++kk;
  float out[3] = {0.f, 0.f, 0.f}, var = 0.f;
  bool ok = false;
  if (kk >= 2) {
    const double px = (double)pts[3 * i], py = (double)pts[3 * i + 1], pz = (double)pts[3 * i + 2];
    const double m = (double)(kk + 1);
    double sx = px, sy = py, sz = pz;
    for (int u = 0; u < kk; ++u) {
      const int64_t j = nbr[i * k + u];
      sx = sx + (double)pts[3 * j], sy = sy + (double)pts[3 * j + 1], sz = sz + (double)pts[3 * j + 2];
    }
    const double mx = sx / m, my = sy / m, mz = sz / m;
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
    for (int u = -1; u < kk; ++u) {
      const int64_t j = u < 0 ? i : (int64_t)nbr[i * k + u];
      const double dx = (double)pts[3 * j] - mx, dy = (double)pts[3 * j + 1] - my, dz = (double)pts[3 * j + 2] - mz;
      a00 = a00 + dx * dx, a01 = a01 + dx * dy, a02 = a02 + dx * dz;
      a11 = a11 + dy * dy, a12 = a12 + dy * dz, a22 = a22 + dz * dz;
    }
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};      // the columns of V
    for (int sweep = 0; sweep < 5; ++sweep) {
      cloud_rotate(a00, a11, a01, a02, a12, v0, v1);      // (p, q, r) = (0, 1, 2)
      cloud_rotate(a00, a22, a02, a01, a12, v0, v2);      // (0, 2, 1)
      cloud_rotate(a11, a22, a12, a01, a02, v1, v2);      // (1, 2, 0)
    }
    const double trace = (a00 + a11) + a22;
    if (trace > 0.0) {
      ok = true;
      double lam = a00, nx = v0[0], ny = v0[1], nz = v0[2];
      if (a11 < lam) lam = a11, nx = v1[0], ny = v1[1], nz = v1[2];
      if (a22 < lam) lam = a22, nx = v2[0], ny = v2[1], nz = v2[2];
      const double len = sqrt((nx * nx + ny * ny) + nz * nz);
      nx = nx / len, ny = ny / len, nz = nz / len;
      bool flip;
      if (toward_mode) {
        const float *t = toward + (toward_mode == 2 ? 3 * i : 0);
        const double tx = (double)t[0] - px, ty = (double)t[1] - py, tz = (double)t[2] - pz;
        flip = (nx * tx + ny * ty) + nz * tz < 0.0;
      } else {
        double big = nx;
        if (fabs(ny) > fabs(big)) big = ny;
        if (fabs(nz) > fabs(big)) big = nz;
        flip = big < 0.0;
      }
      if (flip) nx = -nx, ny = -ny, nz = -nz;
      out[0] = (float)nx, out[1] = (float)ny, out[2] = (float)nz;
      var = (float)((lam > 0.0 ? lam : 0.0) / trace);
    }
  }
  normal[3 * i] = out[0], normal[3 * i + 1] = out[1], normal[3 * i + 2] = out[2];
  variation[i] = var;
  valid[i] = ok;
}

__global__ __launch_bounds__(256) void k_cloud_mean_dist(const int32_t *__restrict__ nbr,
                                                        const float *__restrict__ d2, int64_t n, int k,
                                                        double *__restrict__ mean) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  int kk = 0;
  for (; kk < k && nbr[i * k + kk] >= 0; ++kk) s = s + (double)(float)sqrt((double)d2[i * k + kk]);
  mean[i] = kk ? s / (double)kk : (double)__builtin_inff();
}

// Rule C.5: the cell of a point on the world lattice, 21 bits an axis from the top: z, y, x.
__global__ __launch_bounds__(256) void k_cloud_voxel_keys(const float *__restrict__ pts, int64_t n, float cell,
                                                         uint64_t *__restrict__ keys, int32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    uint64_t key = VKEY_NONE;
    if (cloud_finite(x) && cloud_finite(y) && cloud_finite(z)) {
      const float cx = floorf(__fdiv_rn(x, cell)), cy = floorf(__fdiv_rn(y, cell)), cz = floorf(__fdiv_rn(z, cell));
      const float lim = (float)VOXEL_LIMIT;
      bad = !(fabsf(cx) < lim && fabsf(cy) < lim && fabsf(cz) < lim);
      if (!bad)
        key = (uint64_t)((int)cz + VOXEL_LIMIT - 1) << 42 | (uint64_t)((int)cy + VOXEL_LIMIT - 1) << 21 |
              (uint64_t)((int)cx + VOXEL_LIMIT - 1);
    }
    keys[i] = key;
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(status, SGNN_STATUS_COORD_RANGE);
}

__global__ __launch_bounds__(256) void k_cloud_run_flags(const uint64_t *__restrict__ keys, int64_t n,
                                                        uint8_t *__restrict__ flags) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint64_t k = keys[j];
  flags[j] = k != VKEY_NONE && (j == 0 || keys[j - 1] != k);
}

struct VoxelSum {
  double p[3], nrm[3];
  uint64_t col[4];
};

struct VoxelIn {
  const float *pts, *normals;
  const uint8_t *colors;
  int ncol;
};

struct VoxelRow {
  float p[3], nrm[3];
  uint32_t col[4];
};

__device__ __forceinline__ VoxelRow voxel_load(const VoxelIn &in, int64_t m) {
  VoxelRow r = {};
#pragma unroll
  for (int a = 0; a < 3; ++a) r.p[a] = in.pts[3 * m + a];
  if (in.normals)
#pragma unroll
    for (int a = 0; a < 3; ++a) r.nrm[a] = in.normals[3 * m + a];
  if (in.colors)
#pragma unroll
    for (int a = 0; a < 4; ++a) r.col[a] = a < in.ncol ? in.colors[in.ncol * m + a] : 0;
  return r;
}

__device__ __forceinline__ void voxel_add(VoxelSum &s, const VoxelRow &r) {
#pragma unroll
  for (int a = 0; a < 3; ++a) s.p[a] = s.p[a] + (double)r.p[a], s.nrm[a] = s.nrm[a] + (double)r.nrm[a];
#pragma unroll
  for (int a = 0; a < 4; ++a) s.col[a] += r.col[a];
}

// One lane per run of equal keys.  A lane sums a run of up to LONG_RUN members itself; a longer run is loaded by the
// whole wave, 64 members at a time, and every lane adds the 64 rows in member order (the order of rule C.5) from the
// other lanes' registers, so that the loads of a long run are spread and its sum is the same.
__global__ __launch_bounds__(256) void k_cloud_voxel_reduce(VoxelIn in, int64_t n, const int64_t *__restrict__ order,
                                                           const int32_t *__restrict__ sel, int64_t nruns,
                                                           int64_t nvalid, float *__restrict__ out_pts,
                                                           uint8_t *__restrict__ out_colors,
                                                           float *__restrict__ out_normals,
                                                           int32_t *__restrict__ count, int32_t *__restrict__ first,
                                                           int32_t *__restrict__ cell_of) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool mine = r < nruns;
  int64_t begin = 0, end = 0;
  if (mine) {
    begin = sel[r];
    end = r + 1 < nruns ? (int64_t)sel[r + 1] : nvalid;
    if (begin < 0 || end > nvalid || end < begin) end = begin = 0;      // never for a table of these kernels
  }
  const int64_t len = end - begin;
  VoxelSum sum = {};
  if (mine && len <= LONG_RUN) {
    for (int64_t j = begin; j < end; ++j) {
      const int64_t m = order[j];
      if ((uint64_t)m >= (uint64_t)n) continue;
      voxel_add(sum, voxel_load(in, m));
      cell_of[m] = (int32_t)r;
    }
  }
  unsigned long long todo = __ballot(mine && len > LONG_RUN);
  while (todo) {
    const int owner = __ffsll(todo) - 1;
    todo &= todo - 1;
    const int64_t b0 = __shfl(begin, owner), e0 = __shfl(end, owner), r0 = __shfl(r, owner);
    VoxelSum acc = {};
    for (int64_t base = b0; base < e0; base += 64) {
      const int cnt = (int)min((int64_t)64, e0 - base);
      VoxelRow row = {};
      if (lane < cnt) {
        const int64_t m = order[base + lane];
        if ((uint64_t)m < (uint64_t)n) {
          row = voxel_load(in, m);
          cell_of[m] = (int32_t)r0;
        }
      }
      for (int t = 0; t < cnt; ++t) {
        VoxelRow o;
#pragma unroll
        for (int a = 0; a < 3; ++a) o.p[a] = __shfl(row.p[a], t), o.nrm[a] = __shfl(row.nrm[a], t);
#pragma unroll
        for (int a = 0; a < 4; ++a) o.col[a] = __shfl(row.col[a], t);
        voxel_add(acc, o);
      }
    }
    if (lane == owner) sum = acc;
  }
  if (!mine || len == 0) return;
  const double c = (double)len;
#pragma unroll
  for (int a = 0; a < 3; ++a) out_pts[3 * r + a] = (float)(sum.p[a] / c);
  if (out_normals) {
    const double l2 = (sum.nrm[0] * sum.nrm[0] + sum.nrm[1] * sum.nrm[1]) + sum.nrm[2] * sum.nrm[2];
    const double l = sqrt(l2);
#pragma unroll
    for (int a = 0; a < 3; ++a) out_normals[3 * r + a] = l > 0.0 ? (float)(sum.nrm[a] / l) : 0.f;
  }
  if (out_colors)
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (a < in.ncol) out_colors[in.ncol * r + a] = (uint8_t)((2 * sum.col[a] + (uint64_t)len) / (2 * (uint64_t)len));
  count[r] = (int32_t)len;
  first[r] = (int32_t)order[begin];
}

dim3 cloud_grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

bool cloud_grid_ok(const Grid &g) {
  return g.cell > 0.f && g.cell < __builtin_inff() && g.lox - g.lox == 0.f && g.loy - g.loy == 0.f &&
         g.loz - g.loz == 0.f && g.nx >= 1 && g.ny >= 1 && g.nz >= 1 && g.nx <= MAX_AXIS && g.ny <= MAX_AXIS &&
         g.nz <= MAX_AXIS && (int64_t)g.nx * g.ny * g.nz < (int64_t)CELL_NONE;
}

}  // namespace

SGNN_EXPORT int sgnn_cloud_keys(const float *points, int64_t n, float lox, float loy, float loz, float cell, int nx,
                                int ny, int nz, int64_t *keys, sgnn_stream_t stream) {
  const Grid g = {lox, loy, loz, cell, nx, ny, nz};
  SGNN_CHECK_ARG(n >= 0 && n < LIMIT && cloud_grid_ok(g));
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(points && keys);
  SGNN_LAUNCH(k_cloud_keys, cloud_grid(n), dim3(256), 0, (hipStream_t)stream, points, n, g, (uint64_t *)keys);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_cloud_pack(const float *points, int64_t n, const int64_t *keys, int64_t nfin, int64_t ncell,
                                float *packed, int32_t *start, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && n < LIMIT && nfin >= 0 && nfin <= n && ncell >= 1 && ncell < (int64_t)CELL_NONE);
  SGNN_CHECK_ARG(start && (nfin == 0 || (points && keys && packed)) && ((uintptr_t)packed & 15) == 0);
  SGNN_LAUNCH(k_cloud_pack, cloud_grid(nfin + 1), dim3(256), 0, (hipStream_t)stream, points, n,
              (const uint64_t *)keys, nfin, ncell, (float4 *)packed, start);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

#define CLOUD_KNN(K)                                                                                                 \
  do {                                                                                                               \
    if (self)                                                                                                        \
      SGNN_LAUNCH((k_cloud_knn<K, true>), cloud_grid(nq), dim3(256), 0, s, g, (const float4 *)packed, start, queries, \
                  (const uint64_t *)qkeys, nq, nrows, k, limit2, idx, d2);                                           \
    else                                                                                                             \
      SGNN_LAUNCH((k_cloud_knn<K, false>), cloud_grid(nq), dim3(256), 0, s, g, (const float4 *)packed, start,        \
                  queries, (const uint64_t *)qkeys, nq, nrows, k, limit2, idx, d2);                                  \
  } while (0)

SGNN_EXPORT int sgnn_cloud_knn(const float *packed, int64_t nfin, const int32_t *start, float lox, float loy, float loz,
                               float cell, int nx, int ny, int nz, const float *queries, const int64_t *qkeys,
                               int64_t nq, int64_t nrows, int k, float limit2, int32_t *idx, float *d2,
                               sgnn_stream_t stream) {
  const Grid g = {lox, loy, loz, cell, nx, ny, nz};
  const bool self = queries == nullptr;
  SGNN_CHECK_ARG(nfin >= 0 && nfin < LIMIT && nq >= 0 && nq < LIMIT && nrows >= 0 && nrows < LIMIT && cloud_grid_ok(g));
  SGNN_CHECK_ARG(k >= 1 && k <= 32 && nrows * k < LIMIT && limit2 >= 0.f);
  SGNN_CHECK_ARG(self ? nq == nfin && nrows >= nfin : (nrows == nq && (nq == 0 || qkeys)));
  if (nq == 0) return SGNN_OK;
  SGNN_CHECK_ARG(start && idx && d2 && (nfin == 0 || packed) && ((uintptr_t)packed & 15) == 0);
  const hipStream_t s = (hipStream_t)stream;
  if (k == 1) CLOUD_KNN(1);
  else if (k <= 8) CLOUD_KNN(8);
  else if (k <= 16) CLOUD_KNN(16);
  else CLOUD_KNN(32);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_cloud_radius_count(const float *packed, int64_t nfin, const int32_t *start, float lox, float loy,
                                        float loz, float cell, int nx, int ny, int nz, const float *queries,
                                        const int64_t *qkeys, int64_t nq, float limit2, int32_t *count,
                                        sgnn_stream_t stream) {
  const Grid g = {lox, loy, loz, cell, nx, ny, nz};
  SGNN_CHECK_ARG(nfin >= 0 && nfin < LIMIT && nq >= 0 && nq < LIMIT && cloud_grid_ok(g) && limit2 >= 0.f);
  if (nq == 0) return SGNN_OK;
  SGNN_CHECK_ARG(start && queries && qkeys && count && (nfin == 0 || packed) && ((uintptr_t)packed & 15) == 0);
  SGNN_LAUNCH(k_cloud_radius<false>, cloud_grid(nq), dim3(256), 0, (hipStream_t)stream, g, (const float4 *)packed,
              start, queries, (const uint64_t *)qkeys, nq, limit2, count, (const int64_t *)nullptr,
              (uint64_t *)nullptr);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_cloud_radius_fill(const float *packed, int64_t nfin, const int32_t *start, float lox, float loy,
                                       float loz, float cell, int nx, int ny, int nz, const float *queries,
                                       const int64_t *qkeys, int64_t nq, float limit2, const int64_t *qstart,
                                       int64_t *out, sgnn_stream_t stream) {
  const Grid g = {lox, loy, loz, cell, nx, ny, nz};
  SGNN_CHECK_ARG(nfin >= 0 && nfin < LIMIT && nq >= 0 && nq < LIMIT && cloud_grid_ok(g) && limit2 >= 0.f);
  if (nq == 0) return SGNN_OK;
  SGNN_CHECK_ARG(start && queries && qkeys && qstart && out && (nfin == 0 || packed) && ((uintptr_t)packed & 15) == 0);
  SGNN_LAUNCH(k_cloud_radius<true>, cloud_grid(nq), dim3(256), 0, (hipStream_t)stream, g, (const float4 *)packed,
              start, queries, (const uint64_t *)qkeys, nq, limit2, (int32_t *)nullptr, qstart, (uint64_t *)out);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_cloud_normals(const float *points, int64_t n, const int32_t *nbr, int k, const float *toward,
                                   int toward_mode, float *normal, float *variation, uint8_t *valid,
                                   sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && n < LIMIT && k >= 1 && k <= 32 && n * k < LIMIT && toward_mode >= 0 && toward_mode <= 2);
  SGNN_CHECK_ARG((toward_mode == 0) == (toward == nullptr));
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(points && nbr && normal && variation && valid);
  SGNN_LAUNCH(k_cloud_normals, cloud_grid(n), dim3(256), 0, (hipStream_t)stream, points, n, nbr, k, toward,
              toward_mode, normal, variation, valid);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_cloud_mean_dist(const int32_t *nbr, const float *d2, int64_t n, int k, double *mean,
                                     sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && n < LIMIT && k >= 1 && k <= 32 && n * k < LIMIT);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(nbr && d2 && mean);
  SGNN_LAUNCH(k_cloud_mean_dist, cloud_grid(n), dim3(256), 0, (hipStream_t)stream, nbr, d2, n, k, mean);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_cloud_voxel_keys(const float *points, int64_t n, float cell, int64_t *keys, int32_t *status,
                                      sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && n < LIMIT && cell > 0.f && cell < __builtin_inff());
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(points && keys && status);
  SGNN_LAUNCH(k_cloud_voxel_keys, cloud_grid(n), dim3(256), 0, (hipStream_t)stream, points, n, cell, (uint64_t *)keys,
              status);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_cloud_run_flags(const int64_t *keys, int64_t n, uint8_t *flags, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && n < LIMIT);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(keys && flags);
  SGNN_LAUNCH(k_cloud_run_flags, cloud_grid(n), dim3(256), 0, (hipStream_t)stream, (const uint64_t *)keys, n, flags);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_cloud_voxel_reduce(const float *points, int64_t n, const uint8_t *colors, int ncol,
                                        const float *normals, const int64_t *order, const int32_t *sel, int64_t nruns,
                                        int64_t nvalid, float *out_points, uint8_t *out_colors, float *out_normals,
                                        int32_t *count, int32_t *first, int32_t *cell_of, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && n < LIMIT && nruns >= 0 && nruns <= nvalid && nvalid <= n);
  SGNN_CHECK_ARG(colors ? (ncol == 3 || ncol == 4) && out_colors : ncol == 0 && !out_colors);
  SGNN_CHECK_ARG((normals == nullptr) == (out_normals == nullptr));
  if (nruns == 0) return SGNN_OK;
  SGNN_CHECK_ARG(points && order && sel && out_points && count && first && cell_of);
  const VoxelIn in = {points, normals, colors, ncol};
  SGNN_LAUNCH(k_cloud_voxel_reduce, cloud_grid(nruns), dim3(256), 0, (hipStream_t)stream, in, n, order, sel, nruns,
              nvalid, out_points, out_colors, out_normals, count, first, cell_of);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
