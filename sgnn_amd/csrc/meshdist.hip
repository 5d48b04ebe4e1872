// Mesh-to-mesh distances (sgnn_amd.meshdist): the exact nearest triangle of a mesh for many query points, and
// area-weighted surface samples.  The rules are listed in INTEGRATION.md section G; that text is the contract, and
// tests/meshdist_ref.py restates it independently in NumPy.
//
// Kernels:
//   k_meshdist_pack    one thread per face: index check, rule 1 (usable), the 48-byte record a, ab, ac and the
//                      face's axis-aligned box.  The query never chases verts[faces[t]].
//   k_meshdist_cells   one thread per face walks the cells its box touches (its whole wave, if they are many):
//                      FILL = false counts them, FILL = true writes the face into the CSR lists (the scan between
//                      the two is the caller's)
//   k_meshdist_query   one lane per point: best squared distance, best face and the shell state stay in registers;
//                      shells of increasing Chebyshev radius around the point's (clamped) cell until the bound of
//                      rule 5 proves that no unseen face can win.  A record is three 16-byte loads.
//   k_mesh_sample      one thread per sample: counter hash, binary search in the fp64 cumulative areas, the point.
//
// Built with -ffp-contract=off (Makefile): every product and sum is rounded on its own, divisions and the final
// square root are correctly rounded, so distances match the fp32 restatement bit for bit whatever the grid.
#include <math.h>
#include "common.h"
#include "box_lists.h"  // the cell walk of k_meshdist_cells, shared with voxelize.hip
#include "tri_dist.h"   // rule 2, shared with voxelize.hip

namespace {

// rule 5: the cell of a coordinate, clamped into the grid (NaN -> 0)
__device__ __forceinline__ int cell_of(float x, float lo, float cell, int n) {
  const float q = floorf(__fdiv_rn(x - lo, cell));
  if (!(q >= 0.f)) return 0;
  return q >= (float)n ? n - 1 : (int)q;
}

__global__ __launch_bounds__(256) void k_meshdist_pack(const float *__restrict__ verts, int nverts,
                                                      const int32_t *__restrict__ faces, int ntri,
                                                      float4 *__restrict__ records, float *__restrict__ boxes,
                                                      uint8_t *__restrict__ usable, int32_t *__restrict__ status) {
  const int t = (int)(blockIdx.x * 256 + threadIdx.x);
  bool bad = false;
  if (t < ntri) {
    const int32_t *fc = faces + (int64_t)t * 3;
    const int i0 = fc[0], i1 = fc[1], i2 = fc[2];
    bad = (uint32_t)i0 >= (uint32_t)nverts || (uint32_t)i1 >= (uint32_t)nverts || (uint32_t)i2 >= (uint32_t)nverts;
    V3 a = {0.f, 0.f, 0.f}, ab = a, ac = a;
    bool ok = false;
    const float inf = __int_as_float(0x7F800000);
    float bx[6] = {inf, inf, inf, -inf, -inf, -inf};
    if (!bad) {
      const float *pa = verts + (int64_t)i0 * 3, *pb = verts + (int64_t)i1 * 3, *pc = verts + (int64_t)i2 * 3;
      a = {pa[0], pa[1], pa[2]};
      const V3 b = {pb[0], pb[1], pb[2]}, c = {pc[0], pc[1], pc[2]};
      ab = sub(b, a);
      ac = sub(c, a);
      const float nx = ab.y * ac.z - ab.z * ac.y;
      const float ny = ab.z * ac.x - ab.x * ac.z;
      const float nz = ab.x * ac.y - ab.y * ac.x;
      ok = finite3(a) && finite3(b) && finite3(c) && !(nx == 0.f && ny == 0.f && nz == 0.f);
      if (ok) {
        bx[0] = fminf(a.x, fminf(b.x, c.x));
        bx[1] = fminf(a.y, fminf(b.y, c.y));
        bx[2] = fminf(a.z, fminf(b.z, c.z));
        bx[3] = fmaxf(a.x, fmaxf(b.x, c.x));
        bx[4] = fmaxf(a.y, fmaxf(b.y, c.y));
        bx[5] = fmaxf(a.z, fmaxf(b.z, c.z));
      }
    }
    records[(int64_t)t * 3 + 0] = make_float4(a.x, a.y, a.z, 0.f);
    records[(int64_t)t * 3 + 1] = make_float4(ab.x, ab.y, ab.z, 0.f);
    records[(int64_t)t * 3 + 2] = make_float4(ac.x, ac.y, ac.z, 0.f);
#pragma unroll
    for (int k = 0; k < 6; ++k) boxes[(int64_t)t * 6 + k] = bx[k];
    usable[t] = ok ? 1 : 0;
  }
  if (status && __ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(status, SGNN_STATUS_COORD_RANGE);
}

template <bool FILL>
__global__ __launch_bounds__(256) void k_meshdist_cells(const float *__restrict__ boxes, int ntri, float lox, float loy,
                                                       float loz, float cell, int nx, int ny, int nz,
                                                       const int32_t *__restrict__ offsets,
                                                       int32_t *__restrict__ counts, int32_t *__restrict__ refs) {
  const int t = (int)(blockIdx.x * 256 + threadIdx.x);
  CellRange r = {0, 0, 0, 0, 0, 0};
  if (t < ntri) {
    const float *bx = boxes + (int64_t)t * 6;
    if (bx[0] <= bx[3]) {                                         // false for an ignored face
      r.x0 = cell_of(bx[0], lox, cell, nx);
      r.y0 = cell_of(bx[1], loy, cell, ny);
      r.z0 = cell_of(bx[2], loz, cell, nz);
      r.sx = cell_of(bx[3], lox, cell, nx) - r.x0 + 1;
      r.sy = cell_of(bx[4], loy, cell, ny) - r.y0 + 1;
      r.sz = cell_of(bx[5], loz, cell, nz) - r.z0 + 1;
    }
  }
  list_in_cells<FILL>(r, t, nx, ny, offsets, counts, refs);      // every lane: it holds a ballot
}

template <bool COUNT>
__global__ __launch_bounds__(256) void k_meshdist_query(const float *__restrict__ points, int64_t npts,
                                                       const float4 *__restrict__ records,
                                                       const int32_t *__restrict__ offsets,
                                                       const int32_t *__restrict__ refs, float lox, float loy,
                                                       float loz, float hix, float hiy, float hiz, float cell, int nx,
                                                       int ny, int nz, float max_dist, float *__restrict__ dist,
                                                       int32_t *__restrict__ face,
                                                       unsigned long long *__restrict__ counters) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float inf = __int_as_float(0x7F800000);
  unsigned long long ncell = 0, npair = 0;
  if (i < npts) {
    const V3 p = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
    float best = inf;
    int bt = -1;
    if (finite3(p)) {
      const int cx = cell_of(p.x, lox, cell, nx), cy = cell_of(p.y, loy, cell, ny), cz = cell_of(p.z, loz, cell, nz);
      const float m = fmaxf(fmaxf(fmaxf(fabsf(p.x - lox), fabsf(p.x - hix)), fmaxf(fabsf(p.y - loy), fabsf(p.y - hiy))),
                            fmaxf(fabsf(p.z - loz), fabsf(p.z - hiz)));
      const float slack = m * 3.814697265625e-06f;                // 2^-18
      const int rmax = max(max(max(cx, nx - 1 - cx), max(cy, ny - 1 - cy)), max(cz, nz - 1 - cz));
      auto visit = [&](int c) {
        const int beg = offsets[c], end = offsets[c + 1];
        if (COUNT) {
          ++ncell;
          npair += (unsigned long long)(end - beg);
        }
        for (int k = beg; k < end; ++k) {
          const int t = refs[k];
          const float4 ra = records[(int64_t)t * 3], rb = records[(int64_t)t * 3 + 1], rc = records[(int64_t)t * 3 + 2];
          const float d2 = tri_dist2(p, {ra.x, ra.y, ra.z}, {rb.x, rb.y, rb.z}, {rc.x, rc.y, rc.z});
          if (d2 < best || (d2 == best && t < bt)) {
            best = d2;
            bt = t;
          }
        }
      };
      for (int r = 0;; ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1);
        for (int z = z0; z <= z1; ++z)
          for (int y = y0; y <= y1; ++y) {
            const int row = (z * ny + y) * nx;
            if (z - cz == r || cz - z == r || y - cy == r || cy - y == r) {
              for (int x = x0; x <= x1; ++x) visit(row + x);
            } else {
              if (cx - r >= 0) visit(row + cx - r);
              if (cx + r < nx) visit(row + cx + r);               // r > 0 here
            }
          }
        if (r >= rmax) break;                                     // the block is the whole grid
        float g = inf;
        if (cx - r > 0) g = fminf(g, p.x - (lox + (float)(cx - r) * cell));
        if (cx + r < nx - 1) g = fminf(g, (lox + (float)(cx + r + 1) * cell) - p.x);
        if (cy - r > 0) g = fminf(g, p.y - (loy + (float)(cy - r) * cell));
        if (cy + r < ny - 1) g = fminf(g, (loy + (float)(cy + r + 1) * cell) - p.y);
        if (cz - r > 0) g = fminf(g, p.z - (loz + (float)(cz - r) * cell));
        if (cz + r < nz - 1) g = fminf(g, (loz + (float)(cz + r + 1) * cell) - p.z);
        const float bound = g - slack;
        if (bound > 0.f && (best < bound * bound || bound > max_dist)) break;
      }
    }
    // correctly rounded: the fp64 root of an fp32 number, rounded once more, is the nearest fp32 (53 >= 2 * 24 + 2)
    float d = (float)sqrt((double)best);
    if (!(d <= max_dist)) {
      d = inf;
      bt = -1;
    }
    dist[i] = d;
    face[i] = bt;
  }
  if (COUNT) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      ncell += __shfl_xor(ncell, off);
      npair += __shfl_xor(npair, off);
    }
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(counters + 0, ncell);
      atomicAdd(counters + 1, npair);
    }
  }
}

__device__ __forceinline__ uint32_t frac24(uint64_t base, uint64_t counter) {
  return (uint32_t)(sgnn_hash64(base + counter) >> 40);
}

__global__ __launch_bounds__(256) void k_mesh_sample(const float4 *__restrict__ records, const double *__restrict__ cum,
                                                    int ntri, int last_usable, int64_t n, uint64_t base,
                                                    float *__restrict__ pts, int32_t *__restrict__ fid) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  // one stratum offset for all samples (the fraction of sample 0, k = 0): per-face counts stay within 1 of n area / A
  const uint32_t m0 = frac24(base, 0), m1 = frac24(base, 3 * (uint64_t)i + 1), m2 = frac24(base, 3 * (uint64_t)i + 2);
  const double x = (((double)i + (double)m0 * 0x1p-24) / (double)n) * cum[ntri - 1];
  int lo = 0, hi = ntri;                                          // first t with cum[t] > x
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (cum[mid] > x) hi = mid; else lo = mid + 1;
  }
  const int t = min(lo, last_usable);
  const bool reflect = m1 + m2 > (1u << 24);
  const float u1 = (float)(reflect ? (1u << 24) - m1 : m1) * 0x1p-24f;
  const float u2 = (float)(reflect ? (1u << 24) - m2 : m2) * 0x1p-24f;
  const float4 a = records[(int64_t)t * 3], ab = records[(int64_t)t * 3 + 1], ac = records[(int64_t)t * 3 + 2];
  pts[i * 3 + 0] = (a.x + u1 * ab.x) + u2 * ac.x;
  pts[i * 3 + 1] = (a.y + u1 * ab.y) + u2 * ac.y;
  pts[i * 3 + 2] = (a.z + u1 * ab.z) + u2 * ac.z;
  fid[i] = t;
}

bool grid_ok(float cell, int nx, int ny, int nz) {
  return cell > 0.f && nx >= 1 && ny >= 1 && nz >= 1 && (int64_t)nx * ny * nz < ((int64_t)1 << 31);
}

}  // namespace

SGNN_EXPORT int sgnn_meshdist_pack(const float *verts, int nverts, const int32_t *faces, int ntri, float *records,
                                   float *boxes, uint8_t *usable, int32_t *status, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nverts >= 0 && ntri >= 0 && (int64_t)ntri * 3 < ((int64_t)1 << 31));
  if (ntri == 0) return SGNN_OK;
  SGNN_CHECK_ARG(faces && records && boxes && usable && (nverts == 0 || verts));
  SGNN_CHECK_ARG(((uintptr_t)records & 15) == 0);
  SGNN_LAUNCH(k_meshdist_pack, dim3((ntri + 255) / 256), dim3(256), 0, (hipStream_t)stream, verts, nverts, faces, ntri,
              reinterpret_cast<float4 *>(records), boxes, usable, status);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_meshdist_count(const float *boxes, int ntri, float lox, float loy, float loz, float cell, int nx,
                                    int ny, int nz, int32_t *counts, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(ntri >= 0 && grid_ok(cell, nx, ny, nz));
  if (ntri == 0) return SGNN_OK;
  SGNN_CHECK_ARG(boxes && counts);
  SGNN_LAUNCH(k_meshdist_cells<false>, dim3((ntri + 255) / 256), dim3(256), 0, (hipStream_t)stream, boxes, ntri, lox,
              loy, loz, cell, nx, ny, nz, (const int32_t *)nullptr, counts, (int32_t *)nullptr);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_meshdist_fill(const float *boxes, int ntri, float lox, float loy, float loz, float cell, int nx,
                                   int ny, int nz, const int32_t *offsets, int32_t *cursor, int32_t *refs,
                                   sgnn_stream_t stream) {
  SGNN_CHECK_ARG(ntri >= 0 && grid_ok(cell, nx, ny, nz));
  if (ntri == 0) return SGNN_OK;
  SGNN_CHECK_ARG(boxes && offsets && cursor && refs);
  SGNN_LAUNCH(k_meshdist_cells<true>, dim3((ntri + 255) / 256), dim3(256), 0, (hipStream_t)stream, boxes, ntri, lox,
              loy, loz, cell, nx, ny, nz, offsets, cursor, refs);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_meshdist_query(const float *points, int64_t npts, const float *records, const int32_t *offsets,
                                    const int32_t *refs, float lox, float loy, float loz, float hix, float hiy,
                                    float hiz, float cell, int nx, int ny, int nz, float max_dist, float *dist,
                                    int32_t *face, int64_t *counters, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(npts >= 0 && npts < ((int64_t)1 << 31) * 256 && grid_ok(cell, nx, ny, nz) && max_dist >= 0.f);
  if (npts == 0) return SGNN_OK;
  SGNN_CHECK_ARG(points && records && offsets && refs && dist && face);
  SGNN_CHECK_ARG(((uintptr_t)records & 15) == 0);
  const dim3 grid((unsigned)((npts + 255) / 256));
  const float4 *rec = reinterpret_cast<const float4 *>(records);
  if (counters)
    SGNN_LAUNCH(k_meshdist_query<true>, grid, dim3(256), 0, (hipStream_t)stream, points, npts, rec, offsets, refs, lox,
                loy, loz, hix, hiy, hiz, cell, nx, ny, nz, max_dist, dist, face,
                reinterpret_cast<unsigned long long *>(counters));
  else
    SGNN_LAUNCH(k_meshdist_query<false>, grid, dim3(256), 0, (hipStream_t)stream, points, npts, rec, offsets, refs, lox,
                loy, loz, hix, hiy, hiz, cell, nx, ny, nz, max_dist, dist, face, (unsigned long long *)nullptr);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_mesh_sample(const float *records, const double *cum, int ntri, int last_usable, int64_t n,
                                 int64_t seed, float *pts, int32_t *fid, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31) && ntri >= 0);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(ntri >= 1 && last_usable >= 0 && last_usable < ntri && records && cum && pts && fid);
  SGNN_CHECK_ARG(((uintptr_t)records & 15) == 0);
  // the host-side copy of sgnn_hash64 (a __device__ function): murmur3 finaliser of the seed
  uint64_t k = (uint64_t)seed;
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  SGNN_LAUNCH(k_mesh_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
              reinterpret_cast<const float4 *>(records), cum, ntri, last_usable, n, k, pts, fid);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
