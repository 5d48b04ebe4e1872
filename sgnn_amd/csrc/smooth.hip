// Mesh fairing: vertex adjacency, umbrella (Laplacian / Taubin) steps, face and vertex normals and two-stage
// normal-filter denoising (include/sgnn_hip.h, "Mesh fairing"; rules in INTEGRATION.md section Y, restated on the host
// in tests/smooth_ref.py).
//
// This file is compiled with -ffp-contract=off and uses only fp32 + - *, __fdiv_rn and the correctly rounded root,
// each rounded once, in the order section Y writes down: the NumPy restatement gives the same bits.  No floating-point atomics and no
// cross-lane reduction: every vertex's and every face's sums are taken by one lane, in ascending list order.
//
//   k_smooth_keys        one thread per face: its six directed keys (src << 32 | dst), or KEY_NONE six times (rules 1, 2)
//   k_smooth_run_flags   one thread per sorted key: 1 where a run of equal keys begins
//   k_smooth_runs        one thread per run: source, neighbour and the run length clamped to 255
//   k_smooth_classify    one thread per vertex: its kind from the multiplicities of its run (rule 3)
//   k_smooth_step        one lane per vertex: one umbrella step with factor f (rules 4 to 7)
//   k_smooth_face_normals, k_smooth_corners, k_smooth_vertex_normals       rules 9 and 10
//   k_smooth_filter      one lane per face: one pass of the face-normal filter (rule 11)
//   k_smooth_update      one lane per vertex: one pass of the vertex update (rule 12)
//
// Every pass is a gather bound by latency: about six rows of 12 bytes per vertex, near one another for a mesh in raster
// order.  A lane walks its list in chunks of four so that four rows are in flight; the additions stay in list order.
#include "common.h"

namespace {

constexpr int64_t LIMIT = (int64_t)1 << 31;
constexpr uint64_t KEY_NONE = 0x7FFFFFFFFFFFFFFFull;      // sorts behind every key: a source is below 2^31
enum { KIND_ISOLATED = 0, KIND_INTERIOR = 1, KIND_BOUNDARY = 2, KIND_NONMANIFOLD = 3 };
enum { MODE_FIXED = 0, MODE_CURVE = 1, MODE_FREE = 2 };
enum { FACE_OK = 0, FACE_REPEATED = 1, FACE_RANGE = 2 };

__device__ __forceinline__ int smooth_face(const int32_t *__restrict__ faces, int64_t t, int nverts, int (&v)[3]) {
  v[0] = faces[3 * t], v[1] = faces[3 * t + 1], v[2] = faces[3 * t + 2];
  if (!((uint32_t)v[0] < (uint32_t)nverts && (uint32_t)v[1] < (uint32_t)nverts && (uint32_t)v[2] < (uint32_t)nverts))
    return FACE_RANGE;
  return (v[0] == v[1] || v[1] == v[2] || v[0] == v[2]) ? FACE_REPEATED : FACE_OK;
}

__device__ __forceinline__ bool smooth_finite(float x) { return fabsf(x) < __builtin_inff(); }      // false for a NaN

__device__ __forceinline__ void smooth_raise(bool bad, int32_t *status) {
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(status, SGNN_STATUS_COORD_RANGE);
}

__global__ __launch_bounds__(256) void k_smooth_keys(const int32_t *__restrict__ faces, int ntri, int nverts,
                                                    uint64_t *__restrict__ keys, int32_t *status) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (t < ntri) {
    int v[3];
    const int what = smooth_face(faces, t, nverts, v);
    bad = what == FACE_RANGE;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint64_t a = (uint64_t)(uint32_t)v[k], b = (uint64_t)(uint32_t)v[k == 2 ? 0 : k + 1];
      keys[6 * t + 2 * k] = what == FACE_OK ? (a << 32 | b) : KEY_NONE;
      keys[6 * t + 2 * k + 1] = what == FACE_OK ? (b << 32 | a) : KEY_NONE;
    }
  }
  smooth_raise(bad, status);
}

__global__ __launch_bounds__(256) void k_smooth_run_flags(const uint64_t *__restrict__ keys, int64_t n,
                                                         uint8_t *__restrict__ flags) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint64_t k = keys[j];
  flags[j] = k != KEY_NONE && (j == 0 || keys[j - 1] != k);
}

__global__ __launch_bounds__(256) void k_smooth_runs(const uint64_t *__restrict__ keys, int64_t n,
                                                    const int32_t *__restrict__ sel, int64_t nruns,
                                                    int32_t *__restrict__ source, int32_t *__restrict__ neighbor,
                                                    uint8_t *__restrict__ mult) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= nruns) return;
  const int64_t j = sel[r];
  if (j < 0 || j >= n) return;
  const uint64_t key = keys[j];
  int64_t end;
  if (r + 1 < nruns) {
    end = sel[r + 1];
  } else {      // the last run ends where the keys of degenerate faces begin, or at n
    end = j + 1;
    while (end < n && keys[end] == key) ++end;
  }
  const int64_t len = end - j;
  source[r] = (int32_t)(key >> 32);
  neighbor[r] = (int32_t)(key & 0xFFFFFFFFu);
  mult[r] = (uint8_t)(len > 255 ? 255 : len);
}

__global__ __launch_bounds__(256) void k_smooth_classify(const int64_t *__restrict__ start,
                                                        const uint8_t *__restrict__ mult, int nverts,
                                                        uint8_t *__restrict__ kind) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nverts) return;
  const int64_t e0 = start[i], e1 = start[i + 1];
  bool open = false, many = false;
  for (int64_t e = e0; e < e1; ++e) {
    const int m = mult[e];
    open |= m == 1;
    many |= m > 2;
  }
  kind[i] = e0 >= e1 ? KIND_ISOLATED : many ? KIND_NONMANIFOLD : open ? KIND_BOUNDARY : KIND_INTERIOR;
}

struct Row {
  float x, y, z;
};

template <int S>
__device__ __forceinline__ Row smooth_load(const float *__restrict__ p, int64_t i) {
  if (S == 4) {
    const float4 q = *reinterpret_cast<const float4 *>(p + 4 * i);
    return Row{q.x, q.y, q.z};
  }
  return Row{p[3 * i], p[3 * i + 1], p[3 * i + 2]};
}

template <int S>
__device__ __forceinline__ void smooth_store(float *__restrict__ p, int64_t i, Row r) {
  if (S == 4) {
    *reinterpret_cast<float4 *>(p + 4 * i) = make_float4(r.x, r.y, r.z, 0.f);
  } else {
    p[3 * i] = r.x, p[3 * i + 1] = r.y, p[3 * i + 2] = r.z;
  }
}

// Section Y, rules 4 to 7.  S: floats per row of xin and xout (3, or 4 with the last one unused).
template <int S>
__global__ __launch_bounds__(256) void k_smooth_step(const float *__restrict__ xin, float *__restrict__ xout, int nverts,
                                                    const int64_t *__restrict__ start,
                                                    const int32_t *__restrict__ neighbor,
                                                    const uint8_t *__restrict__ mult, const uint8_t *__restrict__ kind,
                                                    const uint8_t *__restrict__ fixed, int mode, float f,
                                                    int32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (i < nverts) {
    Row x = smooth_load<S>(xin, i);
    bad = !(smooth_finite(x.x) && smooth_finite(x.y) && smooth_finite(x.z));
    const int kd = kind[i];
    const bool moves = (kd == KIND_INTERIOR || (kd == KIND_BOUNDARY && mode != MODE_FIXED)) && !(fixed && fixed[i]);
    const bool rim = kd == KIND_BOUNDARY && mode == MODE_CURVE;      // only over edges of multiplicity 1
    if (moves) {
      Row s = {0.f, 0.f, 0.f};
      int cnt = 0;
      const int64_t e1 = start[i + 1];
      for (int64_t e = start[i]; e < e1; e += 4) {
        int j[4];
        Row p[4] = {};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          j[u] = -1;
          if (e + u < e1 && !(rim && mult[e + u] != 1)) j[u] = neighbor[e + u];
          if ((uint32_t)j[u] >= (uint32_t)nverts) j[u] = -1;      // never for a table of these kernels
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (j[u] >= 0) p[u] = smooth_load<S>(xin, j[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (j[u] < 0) continue;
          if (cnt == 0) s = p[u];
          else s.x = s.x + p[u].x, s.y = s.y + p[u].y, s.z = s.z + p[u].z;
          ++cnt;
        }
      }
      if (cnt > 0) {
        const float d = (float)cnt;
        x.x = x.x + f * (__fdiv_rn(s.x, d) - x.x);
        x.y = x.y + f * (__fdiv_rn(s.y, d) - x.y);
        x.z = x.z + f * (__fdiv_rn(s.z, d) - x.z);
      }
    }
    smooth_store<S>(xout, i, x);
  }
  if (status) smooth_raise(bad, status);
}

__device__ __forceinline__ Row smooth_cross(Row a, Row b, Row c) {
  const float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
  const float wx = c.x - a.x, wy = c.y - a.y, wz = c.z - a.z;
  return Row{uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx};
}

// c / len, or `other` where len is not above 0.  len is the correctly rounded fp32 root, taken as the fp64 root rounded
// once more (exact for fp32 arguments): the fp32 root of the device library is not correctly rounded (geom.h).
__device__ __forceinline__ Row smooth_unit(Row c, Row other) {
  const float len = (float)sqrt((double)((c.x * c.x + c.y * c.y) + c.z * c.z));
  if (!(len > 0.f)) return other;
  return Row{__fdiv_rn(c.x, len), __fdiv_rn(c.y, len), __fdiv_rn(c.z, len)};
}

__global__ __launch_bounds__(256) void k_smooth_face_normals(const float *__restrict__ verts, int nverts,
                                                            const int32_t *__restrict__ faces, int ntri, int unit,
                                                            float *__restrict__ out, int32_t *status) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (t < ntri) {
    int v[3];
    const int what = smooth_face(faces, t, nverts, v);
    bad = what == FACE_RANGE;
    Row n = {0.f, 0.f, 0.f};
    if (what == FACE_OK) {
      n = smooth_cross(smooth_load<3>(verts, v[0]), smooth_load<3>(verts, v[1]), smooth_load<3>(verts, v[2]));
      if (unit) n = smooth_unit(n, Row{0.f, 0.f, 0.f});
    }
    smooth_store<3>(out, t, n);
  }
  if (status) smooth_raise(bad, status);
}

__global__ __launch_bounds__(256) void k_smooth_corners(const int32_t *__restrict__ faces, int ntri, int nverts,
                                                       int32_t *__restrict__ ckeys, int32_t *status) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (t < ntri) {
    int v[3];
    const int what = smooth_face(faces, t, nverts, v);
    bad = what == FACE_RANGE;
#pragma unroll
    for (int k = 0; k < 3; ++k) ckeys[3 * t + k] = what == FACE_OK ? v[k] : nverts;      // list nverts: nobody reads it
  }
  smooth_raise(bad, status);
}

// the face of corner order[j], or -1 (never for an order of these kernels)
__device__ __forceinline__ int64_t smooth_corner_face(const int64_t *__restrict__ order, int64_t j, int ntri) {
  const int64_t t = order[j] / 3;
  return t >= 0 && t < ntri ? t : -1;
}

__global__ __launch_bounds__(256) void k_smooth_vertex_normals(const float *__restrict__ raw, int ntri,
                                                              const int64_t *__restrict__ order,
                                                              const int64_t *__restrict__ cstart, int nverts,
                                                              float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nverts) return;
  Row s = {0.f, 0.f, 0.f};
  for (int64_t j = cstart[i], j1 = cstart[i + 1]; j < j1; ++j) {
    const int64_t t = smooth_corner_face(order, j, ntri);
    if (t < 0) continue;
    const Row c = smooth_load<3>(raw, t);
    s.x = s.x + c.x, s.y = s.y + c.y, s.z = s.z + c.z;
  }
  smooth_store<3>(out, i, smooth_unit(s, Row{0.f, 0.f, 0.f}));
}

// Section Y, rule 11.
__global__ __launch_bounds__(256) void k_smooth_filter(const float *__restrict__ nin, float *__restrict__ nout,
                                                      const int32_t *__restrict__ faces, int ntri, int nverts,
                                                      const int64_t *__restrict__ order,
                                                      const int64_t *__restrict__ cstart, float threshold) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ntri) return;
  const Row n = smooth_load<3>(nin, i);
  int v[3];
  if (smooth_face(faces, i, nverts, v) != FACE_OK) {
    smooth_store<3>(nout, i, n);
    return;
  }
  Row s = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    for (int64_t j = cstart[v[k]], j1 = cstart[v[k] + 1]; j < j1; ++j) {
      const int64_t t = smooth_corner_face(order, j, ntri);
      if (t < 0) continue;
      if (k > 0) {      // a face on an earlier corner of i has been counted there
        const int a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
        if (a == v[0] || b == v[0] || c == v[0]) continue;
        if (k > 1 && (a == v[1] || b == v[1] || c == v[1])) continue;
      }
      const Row m = smooth_load<3>(nin, t);
      const float u = ((n.x * m.x + n.y * m.y) + n.z * m.z) - threshold;
      const float w = u > 0.f ? u * u : 0.f;
      s.x = s.x + w * m.x, s.y = s.y + w * m.y, s.z = s.z + w * m.z;
    }
  }
  smooth_store<3>(nout, i, smooth_unit(s, n));
}

// Section Y, rule 12.
__global__ __launch_bounds__(256) void k_smooth_update(const float *__restrict__ xin, float *__restrict__ xout,
                                                      int nverts, const int32_t *__restrict__ faces, int ntri,
                                                      const float *__restrict__ normals,
                                                      const int64_t *__restrict__ order,
                                                      const int64_t *__restrict__ cstart,
                                                      const uint8_t *__restrict__ kind,
                                                      const uint8_t *__restrict__ fixed, int32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (i < nverts) {
    Row x = smooth_load<3>(xin, i);
    bad = !(smooth_finite(x.x) && smooth_finite(x.y) && smooth_finite(x.z));
    const int kd = kind[i];
    if ((kd == KIND_INTERIOR || kd == KIND_BOUNDARY) && !(fixed && fixed[i])) {
      Row s = {0.f, 0.f, 0.f};
      int cnt = 0;
      for (int64_t j = cstart[i], j1 = cstart[i + 1]; j < j1; ++j) {
        const int64_t t = smooth_corner_face(order, j, ntri);
        int v[3];
        if (t < 0 || smooth_face(faces, t, nverts, v) != FACE_OK) continue;
        const Row n = smooth_load<3>(normals, t);
        if (n.x == 0.f && n.y == 0.f && n.z == 0.f) continue;
        const Row a = smooth_load<3>(xin, v[0]), b = smooth_load<3>(xin, v[1]), c = smooth_load<3>(xin, v[2]);
        const float dx = __fdiv_rn((a.x + b.x) + c.x, 3.f) - x.x;
        const float dy = __fdiv_rn((a.y + b.y) + c.y, 3.f) - x.y;
        const float dz = __fdiv_rn((a.z + b.z) + c.z, 3.f) - x.z;
        const float d = (n.x * dx + n.y * dy) + n.z * dz;
        s.x = s.x + n.x * d, s.y = s.y + n.y * d, s.z = s.z + n.z * d;
        ++cnt;
      }
      if (cnt > 0) {
        const float d = (float)cnt;
        x.x = x.x + __fdiv_rn(s.x, d), x.y = x.y + __fdiv_rn(s.y, d), x.z = x.z + __fdiv_rn(s.z, d);
      }
    }
    smooth_store<3>(xout, i, x);
  }
  if (status) smooth_raise(bad, status);
}

inline dim3 smooth_grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

SGNN_EXPORT int sgnn_smooth_keys(const int32_t *faces, int ntri, int nverts, int64_t *keys, int32_t *status,
                                 sgnn_stream_t stream) {
  SGNN_CHECK_ARG(ntri >= 0 && nverts >= 0 && (int64_t)ntri * 6 < LIMIT);
  if (ntri == 0) return SGNN_OK;
  SGNN_CHECK_ARG(faces && keys && status);
  SGNN_LAUNCH(k_smooth_keys, smooth_grid(ntri), dim3(256), 0, (hipStream_t)stream, faces, ntri, nverts,
              (uint64_t *)keys, status);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_smooth_run_flags(const int64_t *keys, int64_t n, uint8_t *flags, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && n < LIMIT);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(keys && flags);
  SGNN_LAUNCH(k_smooth_run_flags, smooth_grid(n), dim3(256), 0, (hipStream_t)stream, (const uint64_t *)keys, n, flags);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_smooth_runs(const int64_t *keys, int64_t n, const int32_t *sel, int64_t nruns, int32_t *source,
                                 int32_t *neighbor, uint8_t *mult, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && n < LIMIT && nruns >= 0 && nruns <= n);
  if (nruns == 0) return SGNN_OK;
  SGNN_CHECK_ARG(keys && sel && source && neighbor && mult);
  SGNN_LAUNCH(k_smooth_runs, smooth_grid(nruns), dim3(256), 0, (hipStream_t)stream, (const uint64_t *)keys, n, sel,
              nruns, source, neighbor, mult);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_smooth_classify(const int64_t *start, const uint8_t *mult, int nverts, uint8_t *kind,
                                     sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nverts >= 0);
  if (nverts == 0) return SGNN_OK;
  SGNN_CHECK_ARG(start && mult && kind);
  SGNN_LAUNCH(k_smooth_classify, smooth_grid(nverts), dim3(256), 0, (hipStream_t)stream, start, mult, nverts, kind);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_smooth_step(const float *xin, float *xout, int nverts, int stride, const int64_t *start,
                                 const int32_t *neighbor, const uint8_t *mult, const uint8_t *kind,
                                 const uint8_t *fixed, int mode, float f, int32_t *status, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nverts >= 0 && (stride == 3 || stride == 4) && mode >= MODE_FIXED && mode <= MODE_FREE);
  SGNN_CHECK_ARG(f > -__builtin_inff() && f < __builtin_inff());
  if (nverts == 0) return SGNN_OK;
  SGNN_CHECK_ARG(xin && xout && xin != xout && start && neighbor && mult && kind);
  SGNN_CHECK_ARG(stride == 3 || (((uintptr_t)xin | (uintptr_t)xout) & 15) == 0);
  const hipStream_t s = (hipStream_t)stream;
  if (stride == 4)
    SGNN_LAUNCH(k_smooth_step<4>, smooth_grid(nverts), dim3(256), 0, s, xin, xout, nverts, start, neighbor, mult, kind,
                fixed, mode, f, status);
  else
    SGNN_LAUNCH(k_smooth_step<3>, smooth_grid(nverts), dim3(256), 0, s, xin, xout, nverts, start, neighbor, mult, kind,
                fixed, mode, f, status);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_smooth_face_normals(const float *verts, int nverts, const int32_t *faces, int ntri, int unit,
                                         float *out, int32_t *status, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nverts >= 0 && ntri >= 0 && (int64_t)ntri * 3 < LIMIT && (unit == 0 || unit == 1));
  if (ntri == 0) return SGNN_OK;
  SGNN_CHECK_ARG(faces && out && (nverts == 0 || verts));
  SGNN_LAUNCH(k_smooth_face_normals, smooth_grid(ntri), dim3(256), 0, (hipStream_t)stream, verts, nverts, faces, ntri,
              unit, out, status);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_smooth_corners(const int32_t *faces, int ntri, int nverts, int32_t *ckeys, int32_t *status,
                                    sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nverts >= 0 && ntri >= 0 && (int64_t)ntri * 3 < LIMIT);
  if (ntri == 0) return SGNN_OK;
  SGNN_CHECK_ARG(faces && ckeys && status);
  SGNN_LAUNCH(k_smooth_corners, smooth_grid(ntri), dim3(256), 0, (hipStream_t)stream, faces, ntri, nverts, ckeys,
              status);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_smooth_vertex_normals(const float *raw, int ntri, const int64_t *order, const int64_t *cstart,
                                           int nverts, float *out, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nverts >= 0 && ntri >= 0 && (int64_t)ntri * 3 < LIMIT);
  if (nverts == 0) return SGNN_OK;
  SGNN_CHECK_ARG(cstart && out && (ntri == 0 || (raw && order)));
  SGNN_LAUNCH(k_smooth_vertex_normals, smooth_grid(nverts), dim3(256), 0, (hipStream_t)stream, raw, ntri, order, cstart,
              nverts, out);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_smooth_filter(const float *nin, float *nout, const int32_t *faces, int ntri, int nverts,
                                   const int64_t *order, const int64_t *cstart, float threshold, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nverts >= 0 && ntri >= 0 && (int64_t)ntri * 3 < LIMIT);
  SGNN_CHECK_ARG(threshold > -__builtin_inff() && threshold < __builtin_inff());
  if (ntri == 0) return SGNN_OK;
  SGNN_CHECK_ARG(nin && nout && nin != nout && faces && order && cstart);
  SGNN_LAUNCH(k_smooth_filter, smooth_grid(ntri), dim3(256), 0, (hipStream_t)stream, nin, nout, faces, ntri, nverts,
              order, cstart, threshold);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_smooth_update(const float *xin, float *xout, int nverts, const int32_t *faces, int ntri,
                                   const float *normals, const int64_t *order, const int64_t *cstart,
                                   const uint8_t *kind, const uint8_t *fixed, int32_t *status, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nverts >= 0 && ntri >= 0 && (int64_t)ntri * 3 < LIMIT);
  if (nverts == 0) return SGNN_OK;
  SGNN_CHECK_ARG(xin && xout && xin != xout && cstart && kind && (ntri == 0 || (faces && normals && order)));
  SGNN_LAUNCH(k_smooth_update, smooth_grid(nverts), dim3(256), 0, (hipStream_t)stream, xin, xout, nverts, faces, ntri,
              normals, order, cstart, kind, fixed, status);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
