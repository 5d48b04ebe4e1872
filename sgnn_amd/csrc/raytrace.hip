// Arbitrary rays against a triangle mesh (sgnn_amd.raytrace): the closest hit of every ray, or whether anything lies
// on a segment.  The rules are listed in INTEGRATION.md section W; that text is the contract, and tests/raytrace_ref.py
// restates it independently in NumPy (brute force over all faces).
//
// The mesh is what meshdist.TriangleIndex keeps: the 48-byte records a, ab, ac of sgnn_meshdist_pack and the CSR lists
// of sgnn_meshdist_count / fill, here built from boxes grown by a guard on every side (rule W.4).
//
// Kernel:
//   k_raytrace<ANY, COUNT>   one lane per ray.  The ray is clipped to the grid's box grown by the guard (slab test),
//                            then walks cell to cell; every crossing parameter comes straight from the integer cell
//                            index, never from an accumulated increment.  Best t, u, v, face, the three cell indices and
//                            the three crossing parameters stay in registers; a record is three 16-byte loads.
//                            ANY = false: closest hit, the walk ends once the best t lies in the cells already seen.
//                            ANY = true: per-ray t_max, the walk ends at the first hit.
//
// Built with -ffp-contract=off (Makefile): every product and sum is rounded on its own and the one division per test is
// correctly rounded, so t and uv match the fp32 restatement bit for bit whatever the grid and the order of the rays.
#include <math.h>
#include "common.h"
#include "tri_dist.h"   // V3, sub, dot (section G), finite3

namespace {

__device__ __forceinline__ V3 cross(const V3 &u, const V3 &v) {
  return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}

// rule W.1: Moeller-Trumbore on the record.  Every comparison is written so that a NaN anywhere is a miss.
__device__ __forceinline__ bool ray_face(const V3 &o, const V3 &d, const V3 &a, const V3 &ab, const V3 &ac, bool cull,
                                         float t_min, float t_max, float &t, float &u, float &v) {
  const V3 p = cross(d, ac);
  const float det = dot(ab, p);
  if (cull ? !(det > 0.f) : det == 0.f) return false;
  const float inv = __fdiv_rn(1.f, det);
  const V3 s = sub(o, a);
  u = dot(s, p) * inv;
  const V3 q = cross(s, ab);
  v = dot(d, q) * inv;
  t = dot(ac, q) * inv;
  return u >= 0.f && v >= 0.f && u + v <= 1.f && t > t_min && t < t_max;
}

// the cell of a coordinate, clamped into the grid (the caller has ruled out a NaN)
__device__ __forceinline__ int clamp_cell(float x, float lo, float cell, int n) {
  const float q = floorf(__fdiv_rn(x - lo, cell));
  if (!(q >= 0.f)) return 0;
  return q >= (float)n ? n - 1 : (int)q;
}

struct Axis {
  float o, d, lo;   // the ray and the grid along this axis
  int i, n, step;   // current cell, cells, -1 / 0 / +1
  float next;       // parameter at which the ray leaves cell i along this axis (+inf: never)
};

// rule W.4: the crossing parameter straight from the integer index
__device__ __forceinline__ float crossing(const Axis &a, float cell) {
  if (a.step == 0) return __int_as_float(0x7F800000);
  const float plane = a.lo + (float)(a.i + (a.step > 0 ? 1 : 0)) * cell;
  return __fdiv_rn(plane - a.o, a.d);
}

// one cell on along this axis; false: the ray has left the grid
__device__ __forceinline__ bool advance(Axis &a, float cell) {
  a.i += a.step;
  a.next = crossing(a, cell);
  return a.i >= 0 && a.i < a.n;
}

// the slab of one axis of the grown box; false: the ray never enters it
__device__ __forceinline__ bool slab(float o, float d, float lo, float hi, float &t0, float &t1) {
  if (d == 0.f) return o >= lo && o <= hi;
  const float a = __fdiv_rn(lo - o, d), b = __fdiv_rn(hi - o, d);
  t0 = fmaxf(t0, fminf(a, b));
  t1 = fminf(t1, fmaxf(a, b));
  return true;
}

template <bool ANY, bool COUNT>
__global__ __launch_bounds__(256) void k_raytrace(const float *__restrict__ origins, const float *__restrict__ dirs,
                                                 int64_t nrays, float t_min, float t_max_all,
                                                 const float *__restrict__ t_max_ray,
                                                 const float4 *__restrict__ records, const int32_t *__restrict__ offsets,
                                                 const int32_t *__restrict__ refs, float lox, float loy, float loz,
                                                 float cell, int nx, int ny, int nz, float guard, int cull_back,
                                                 float *__restrict__ out_t, int32_t *__restrict__ out_face,
                                                 float *__restrict__ out_uv, uint8_t *__restrict__ out_hit,
                                                 unsigned long long *__restrict__ counters) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float inf = __int_as_float(0x7F800000);
  unsigned long long ncell = 0, npair = 0;
  if (r < nrays) {
    const V3 o = {origins[r * 3], origins[r * 3 + 1], origins[r * 3 + 2]};
    const V3 d = {dirs[r * 3], dirs[r * 3 + 1], dirs[r * 3 + 2]};
    const float t_max = ANY ? t_max_ray[r] : t_max_all;
    const bool cull = cull_back != 0;
    float best = inf, bu = 0.f, bv = 0.f;
    int bt = -1;
    bool found = false;
    float t0 = t_min, t1 = t_max;
    bool live = finite3(o) && finite3(d) && !(d.x == 0.f && d.y == 0.f && d.z == 0.f) && t_min < t_max;
    live = live && slab(o.x, d.x, lox - guard, (lox + (float)nx * cell) + guard, t0, t1);
    live = live && slab(o.y, d.y, loy - guard, (loy + (float)ny * cell) + guard, t0, t1);
    live = live && slab(o.z, d.z, loz - guard, (loz + (float)nz * cell) + guard, t0, t1);
    if (live && t0 <= t1) {                                        // false for a NaN as well
      // the cell of the entry point o + t0 d; a zero component of d contributes o itself, never 0 * inf
      Axis ax[3] = {{o.x, d.x, lox, 0, nx, d.x > 0.f ? 1 : (d.x < 0.f ? -1 : 0), 0.f},
                    {o.y, d.y, loy, 0, ny, d.y > 0.f ? 1 : (d.y < 0.f ? -1 : 0), 0.f},
                    {o.z, d.z, loz, 0, nz, d.z > 0.f ? 1 : (d.z < 0.f ? -1 : 0), 0.f}};
      bool ok = isfinite(t0);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float p = ax[k].step == 0 ? ax[k].o : ax[k].o + t0 * ax[k].d;
        ok = ok && isfinite(p);
        ax[k].i = clamp_cell(p, ax[k].lo, cell, ax[k].n);
        ax[k].next = crossing(ax[k], cell);
      }
      while (ok) {
        const int c = (ax[2].i * ny + ax[1].i) * nx + ax[0].i;
        const int beg = offsets[c], end = offsets[c + 1];
        if (COUNT) ++ncell;
        for (int k = beg; k < end; ++k) {
          const int f = refs[k];
          const float4 ra = records[(int64_t)f * 3], rb = records[(int64_t)f * 3 + 1], rc = records[(int64_t)f * 3 + 2];
          float t, u, v;
          if (COUNT) ++npair;
          if (!ray_face(o, d, {ra.x, ra.y, ra.z}, {rb.x, rb.y, rb.z}, {rc.x, rc.y, rc.z}, cull, t_min, t_max, t, u, v))
            continue;
          if (ANY) {
            found = true;
            break;
          }
          if (t < best || (t == best && f < bt)) {
            best = t;
            bu = u;
            bv = v;
            bt = f;
          }
        }
        if (ANY && found) break;
        // the axis the ray leaves this cell by: the smallest crossing parameter, x before y before z among equals
        int m = 0;
        float tn = ax[0].next;
        if (ax[1].next < tn) { tn = ax[1].next; m = 1; }
        if (ax[2].next < tn) { tn = ax[2].next; m = 2; }
        // rule W.4: every face that could beat `best` is hit before tn, hence listed in a cell already seen; beyond
        // t1 the ray is outside the grown box or past t_max; a NaN or +inf ends the walk as well
        if (!(tn < t1) || best <= tn) break;
        ok = m == 0 ? advance(ax[0], cell) : (m == 1 ? advance(ax[1], cell) : advance(ax[2], cell));   // constant
      }                                                             // indices: ax stays in registers
    }
    if (ANY) {
      out_hit[r] = found ? 1 : 0;
    } else {
      out_t[r] = best;
      out_face[r] = bt;
      out_uv[r * 2] = bu;
      out_uv[r * 2 + 1] = bv;
    }
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

bool grid_ok(float lox, float loy, float loz, float cell, int nx, int ny, int nz, float guard) {
  return isfinite(lox) && isfinite(loy) && isfinite(loz) && isfinite(cell) && cell > 0.f && isfinite(guard) &&
         guard >= 0.f && nx >= 1 && ny >= 1 && nz >= 1 && (int64_t)nx * ny * nz < ((int64_t)1 << 31);
}

template <bool ANY>
int launch(const float *origins, const float *dirs, int64_t nrays, float t_min, float t_max_all, const float *t_max_ray,
           const float *records, const int32_t *offsets, const int32_t *refs, float lox, float loy, float loz,
           float cell, int nx, int ny, int nz, float guard, int cull_back, float *t, int32_t *face, float *uv,
           uint8_t *hit, int64_t *counters, sgnn_stream_t stream) {
  const dim3 grid((unsigned)((nrays + 255) / 256));
  const float4 *rec = reinterpret_cast<const float4 *>(records);
  unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counters);
  if (counters)
    SGNN_LAUNCH((k_raytrace<ANY, true>), grid, dim3(256), 0, (hipStream_t)stream, origins, dirs, nrays, t_min,
                t_max_all, t_max_ray, rec, offsets, refs, lox, loy, loz, cell, nx, ny, nz, guard, cull_back, t, face, uv,
                hit, cnt);
  else
    SGNN_LAUNCH((k_raytrace<ANY, false>), grid, dim3(256), 0, (hipStream_t)stream, origins, dirs, nrays, t_min,
                t_max_all, t_max_ray, rec, offsets, refs, lox, loy, loz, cell, nx, ny, nz, guard, cull_back, t, face, uv,
                hit, cnt);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

}  // namespace

SGNN_EXPORT int sgnn_raytrace_closest(const float *origins, const float *dirs, int64_t nrays, float t_min, float t_max,
                                      const float *records, const int32_t *offsets, const int32_t *refs, float lox,
                                      float loy, float loz, float cell, int nx, int ny, int nz, float guard,
                                      int cull_back, float *t, int32_t *face, float *uv, int64_t *counters,
                                      sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nrays >= 0 && nrays < ((int64_t)1 << 31) * 256 && grid_ok(lox, loy, loz, cell, nx, ny, nz, guard));
  SGNN_CHECK_ARG(isfinite(t_min) && t_min < t_max && (cull_back == 0 || cull_back == 1));
  if (nrays == 0) return SGNN_OK;
  SGNN_CHECK_ARG(origins && dirs && records && offsets && refs && t && face && uv);
  SGNN_CHECK_ARG(((uintptr_t)records & 15) == 0);
  return launch<false>(origins, dirs, nrays, t_min, t_max, nullptr, records, offsets, refs, lox, loy, loz, cell, nx, ny,
                       nz, guard, cull_back, t, face, uv, nullptr, counters, stream);
}

SGNN_EXPORT int sgnn_raytrace_occluded(const float *origins, const float *dirs, int64_t nrays, float t_min,
                                       const float *t_max, const float *records, const int32_t *offsets,
                                       const int32_t *refs, float lox, float loy, float loz, float cell, int nx, int ny,
                                       int nz, float guard, int cull_back, uint8_t *hit, int64_t *counters,
                                       sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nrays >= 0 && nrays < ((int64_t)1 << 31) * 256 && grid_ok(lox, loy, loz, cell, nx, ny, nz, guard));
  SGNN_CHECK_ARG(isfinite(t_min) && (cull_back == 0 || cull_back == 1));
  if (nrays == 0) return SGNN_OK;
  SGNN_CHECK_ARG(origins && dirs && t_max && records && offsets && refs && hit);
  SGNN_CHECK_ARG(((uintptr_t)records & 15) == 0);
  return launch<true>(origins, dirs, nrays, t_min, 0.f, t_max, records, offsets, refs, lox, loy, loz, cell, nx, ny, nz,
                      guard, cull_back, nullptr, nullptr, nullptr, hit, counters, stream);
}
