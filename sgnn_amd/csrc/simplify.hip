// Mesh simplification by vertex clustering with quadric placement (include/sgnn_hip.h, "Mesh simplification"; rules in
// INTEGRATION.md section K, restated on the host in tests/simplify_ref.py).
//
// This file is compiled with -ffp-contract=off and uses only fp32 - / floor and fp64 + - * /, each rounded once, in the
// order section K writes down: the NumPy restatement gives the same bits.  No floating-point atomics: every cluster's
// sums are taken by one lane, in ascending corner number.
//
//   k_simp_keys     one thread per vertex: the 63-bit cell key (rule 1), or SIMP_EMPTY and the status word
//   k_simp_insert   the first-member table of first_table.h with the 64-bit key in the slot (rule 2)
//   k_simp_lookup   first_of[i] = smallest member of vertex i's cluster, is_first[i]
//   k_simp_corners  one thread per face: corner_first[3t+k] = first_of[faces[t][k]] (rule 3), bad faces -> status
//   (the caller numbers the clusters with sgnn_compact_mask + sgnn_weld_number and remaps / de-duplicates the faces
//    with sgnn_mesh_faces, the shared code of mesh_tables.hip: rule 6)
//   k_simp_mark     used[c] = 1 for every cluster a kept face refers to
//   k_simp_place    one lane per surviving cluster: rule 4's sums over its corners, rule 5's solve, the vertex
//
// All passes are gathers bound by latency; k_simp_place reads nine floats per corner and keeps ~16 doubles per lane.
#include "common.h"
#include "first_table.h"

namespace {

constexpr uint64_t SIMP_EMPTY = SLOT_EMPTY<uint64_t>;    // no key has bit 63 set
constexpr float SIMP_CELLS_AXIS = 2097152.0f;              // 2^21 cells per axis
constexpr int64_t LIMIT = (int64_t)1 << 31;

__global__ __launch_bounds__(256) void k_simp_keys(const float *__restrict__ verts, int64_t nv,
                                                  const float *__restrict__ origin, float cell,
                                                  uint64_t *__restrict__ keys, int32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (i < nv) {
    uint64_t key = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float c = floorf(__fdiv_rn(verts[3 * i + k] - origin[k], cell));
      if (c >= 0.0f && c < SIMP_CELLS_AXIS) key = (key << 21) | (uint64_t)(uint32_t)(int)c;    // a NaN fails both
      else bad = true;
    }
    keys[i] = bad ? SIMP_EMPTY : key;
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(status, SGNN_STATUS_COORD_RANGE);
}

__global__ __launch_bounds__(256) void k_simp_insert(const uint64_t *__restrict__ keys, int64_t nv, uint64_t *tkeys,
                                                    int32_t *tfirst, int64_t cap) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv) return;
  const uint64_t key = keys[i];
  if (key == SIMP_EMPTY) return;
  first_insert(tkeys, tfirst, cap, (int64_t)(sgnn_hash64(key) % (uint64_t)cap), (int32_t)i, key,
               [&](uint64_t k) { return k == key; });
}

__global__ __launch_bounds__(256) void k_simp_lookup(const uint64_t *__restrict__ keys, int64_t nv,
                                                    const uint64_t *__restrict__ tkeys,
                                                    const int32_t *__restrict__ tfirst, int64_t cap,
                                                    int32_t *__restrict__ first_of, uint8_t *__restrict__ is_first) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv) return;
  const uint64_t key = keys[i];
  int32_t f = -1;
  if (key != SIMP_EMPTY) {
    const int64_t home = (int64_t)(sgnn_hash64(key) % (uint64_t)cap);
    f = tfirst[first_find<true>(tkeys, cap, home, [&](uint64_t k) { return k == key; })];  // present: k_simp_insert ran first
  }
  first_of[i] = f;
  is_first[i] = f == (int32_t)i;
}

__device__ __forceinline__ bool simp_face(const int32_t *__restrict__ faces, int64_t t, int nverts, int (&v)[3]) {
  v[0] = faces[3 * t], v[1] = faces[3 * t + 1], v[2] = faces[3 * t + 2];
  return (uint32_t)v[0] < (uint32_t)nverts && (uint32_t)v[1] < (uint32_t)nverts && (uint32_t)v[2] < (uint32_t)nverts;
}

__global__ __launch_bounds__(256) void k_simp_corners(const int32_t *__restrict__ faces, int ntri, int nverts,
                                                     const int32_t *__restrict__ first_of,
                                                     int32_t *__restrict__ corner_first, int32_t *status) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (t < ntri) {
    int v[3], f[3] = {0, 0, 0};
    bad = !simp_face(faces, t, nverts, v);
    if (!bad) {
#pragma unroll
      for (int k = 0; k < 3; ++k) f[k] = first_of[v[k]];
      if (f[0] < 0 || f[1] < 0 || f[2] < 0) f[0] = f[1] = f[2] = 0;      // a vertex without a key: k_simp_keys raised it
    }
    // a face passed over holds vertex 0 three times: in range and degenerate for whoever reads it before the status
#pragma unroll
    for (int k = 0; k < 3; ++k) corner_first[3 * t + k] = f[k];
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(status, SGNN_STATUS_COORD_RANGE);
}

__global__ __launch_bounds__(256) void k_simp_mark(const int32_t *__restrict__ cfaces, int64_t nfaces, int64_t nclust,
                                                  uint8_t *used) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= 3 * nfaces) return;
  const int32_t c = cfaces[e];
  if (c >= 0 && (int64_t)c < nclust) used[c] = 1;      // every writer of a slot stores the same value
}

// Section K, rules 4 and 5, for output vertex p = cluster csel[p].  The order of every sum is the one written there.
template <bool QUADRIC, bool COLORS>
__global__ __launch_bounds__(256) void k_simp_place(const float *__restrict__ verts, int nverts,
                                                   const int32_t *__restrict__ faces, int ntri,
                                                   const uint8_t *__restrict__ colors,
                                                   const int64_t *__restrict__ order, const int64_t *__restrict__ start,
                                                   const int32_t *__restrict__ csel, int64_t nout,
                                                   const int32_t *__restrict__ sel, const uint64_t *__restrict__ keys,
                                                   const float *__restrict__ origin, float cell,
                                                   float *__restrict__ out_verts, uint8_t *__restrict__ out_colors) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= nout) return;
  const int32_t c = csel[p];
  const uint64_t key = keys[sel[c]];
  const double cd = (double)cell;
  double o[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    o[k] = (double)origin[k] + ((double)(int)((key >> (21 * (2 - k))) & 0x1FFFFFu) + 0.5) * cd;
  double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, b0 = 0, b1 = 0, b2 = 0, s0 = 0, s1 = 0, s2 = 0;
  int64_t count = 0, col[3] = {0, 0, 0};
  for (int64_t j = start[c], end = start[c + 1]; j < end; ++j) {
    const int64_t e = order[j];
    const int64_t t = e / 3;
    const int k = (int)(e - 3 * t);
    int v[3];
    if (t < 0 || t >= ntri || !simp_face(faces, t, nverts, v)) continue;
    double q[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int d = 0; d < 3; ++d) q[a][d] = (double)verts[3 * (int64_t)v[a] + d] - o[d];
    if (QUADRIC) {
      const double ux = q[1][0] - q[0][0], uy = q[1][1] - q[0][1], uz = q[1][2] - q[0][2];
      const double wx = q[2][0] - q[0][0], wy = q[2][1] - q[0][1], wz = q[2][2] - q[0][2];
      const double n0 = uy * wz - uz * wy, n1 = uz * wx - ux * wz, n2 = ux * wy - uy * wx;
      const double d = (n0 * q[0][0] + n1 * q[0][1]) + n2 * q[0][2];
      a00 += n0 * n0, a01 += n0 * n1, a02 += n0 * n2, a11 += n1 * n1, a12 += n1 * n2, a22 += n2 * n2;
      b0 += n0 * d, b1 += n1 * d, b2 += n2 * d;
    }
    s0 += q[k][0], s1 += q[k][1], s2 += q[k][2];
    ++count;
    if (COLORS) {
#pragma unroll
      for (int d = 0; d < 3; ++d) col[d] += colors[3 * (int64_t)v[k] + d];
    }
  }
  const double cnt = (double)count;      // >= 1: a surviving face refers to the cluster
  const double m0 = s0 / cnt, m1 = s1 / cnt, m2 = s2 / cnt;
  double x0 = m0, x1 = m1, x2 = m2;
  if (QUADRIC) {
    const double delta = (1e-5 * ((a00 + a11) + a22)) / 3.0;
    if (delta != 0.0) {
      const double r0 = b0 - ((a00 * m0 + a01 * m1) + a02 * m2);
      const double r1 = b1 - ((a01 * m0 + a11 * m1) + a12 * m2);
      const double r2 = b2 - ((a02 * m0 + a12 * m1) + a22 * m2);
      // (A + delta I) y = r by L D L^T
      const double d0 = a00 + delta;
      const double l10 = a01 / d0, l20 = a02 / d0;
      const double d1 = (a11 + delta) - l10 * a01;
      const double u12 = a12 - l20 * a01;
      const double l21 = u12 / d1;
      const double d2 = ((a22 + delta) - l20 * a02) - l21 * u12;
      const double z1 = r1 - l10 * r0;
      const double z2 = (r2 - l20 * r0) - l21 * z1;
      const double y2 = z2 / d2;
      const double y1 = z1 / d1 - l21 * y2;
      const double y0 = (r0 / d0 - l10 * y1) - l20 * y2;
      x0 = m0 + y0, x1 = m1 + y1, x2 = m2 + y2;
      if (!(fabs(x0) <= cd && fabs(x1) <= cd && fabs(x2) <= cd)) x0 = m0, x1 = m1, x2 = m2;
    }
  }
  out_verts[3 * p] = (float)(o[0] + x0);
  out_verts[3 * p + 1] = (float)(o[1] + x1);
  out_verts[3 * p + 2] = (float)(o[2] + x2);
  if (COLORS) {
#pragma unroll
    for (int d = 0; d < 3; ++d) out_colors[3 * p + d] = (uint8_t)((2 * col[d] + count) / (2 * count));
  }
}

}  // namespace

SGNN_EXPORT int sgnn_simp_keys(const float *verts, int64_t nv, const float *origin, float cell, int64_t *keys,
                               int32_t *status, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nv >= 0 && nv < LIMIT && cell > 0.f && cell < __builtin_inff());
  if (nv == 0) return SGNN_OK;
  SGNN_CHECK_ARG(verts && origin && keys && status);
  SGNN_LAUNCH(k_simp_keys, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts, nv, origin,
              cell, (uint64_t *)keys, status);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_simp_clusters(const int64_t *keys, int64_t nv, int64_t *tkeys, int32_t *tfirst, int64_t cap,
                                   int32_t *first_of, uint8_t *is_first, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nv >= 0 && nv < LIMIT && cap >= sgnn_weld_slots(nv) && tkeys && tfirst);
  if (nv == 0) return SGNN_OK;
  SGNN_CHECK_ARG(keys && first_of && is_first);
  const hipStream_t s = (hipStream_t)stream;
  int rc = sgnn_fill32(tkeys, 0xFFFFFFFFu, 2 * cap, s);      // SIMP_EMPTY
  if (rc == SGNN_OK) rc = sgnn_fill32(tfirst, 0x7FFFFFFFu, cap, s);
  if (rc != SGNN_OK) return rc;
  const dim3 grid((unsigned)((nv + 255) / 256));
  SGNN_LAUNCH(k_simp_insert, grid, dim3(256), 0, s, (const uint64_t *)keys, nv, (uint64_t *)tkeys, tfirst, cap);
  SGNN_CHECK_LAUNCH();
  SGNN_LAUNCH(k_simp_lookup, grid, dim3(256), 0, s, (const uint64_t *)keys, nv, (const uint64_t *)tkeys,
              (const int32_t *)tfirst, cap, first_of, is_first);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_simp_corners(const int32_t *faces, int ntri, int nverts, const int32_t *first_of,
                                  int32_t *corner_first, int32_t *status, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(ntri >= 0 && nverts >= 0 && (int64_t)ntri * 3 < LIMIT);
  if (ntri == 0) return SGNN_OK;
  SGNN_CHECK_ARG(faces && corner_first && status && (nverts == 0 || first_of));
  SGNN_LAUNCH(k_simp_corners, dim3((unsigned)((ntri + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, ntri,
              nverts, first_of, corner_first, status);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_simp_mark(const int32_t *cfaces, int64_t nfaces, int64_t nclust, uint8_t *used,
                               sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nfaces >= 0 && 3 * nfaces < LIMIT && nclust >= 0);
  if (nfaces == 0 || nclust == 0) return SGNN_OK;
  SGNN_CHECK_ARG(cfaces && used);
  SGNN_LAUNCH(k_simp_mark, dim3((unsigned)((3 * nfaces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cfaces,
              nfaces, nclust, used);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_simp_place(const float *verts, int nverts, const int32_t *faces, int ntri, const uint8_t *colors,
                                const int64_t *order, const int64_t *start, const int32_t *csel, int64_t nout,
                                const int32_t *sel, const int64_t *keys, const float *origin, float cell, int quadric,
                                float *out_verts, uint8_t *out_colors, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nverts >= 0 && ntri >= 0 && (int64_t)ntri * 3 < LIMIT && nout >= 0 && nout <= nverts);
  SGNN_CHECK_ARG(cell > 0.f && cell < __builtin_inff() && (quadric == 0 || quadric == 1));
  if (nout == 0) return SGNN_OK;
  SGNN_CHECK_ARG(verts && faces && order && start && csel && sel && keys && origin && out_verts);
  SGNN_CHECK_ARG(!colors == !out_colors);
  const dim3 grid((unsigned)((nout + 255) / 256));
  const hipStream_t s = (hipStream_t)stream;
  const uint64_t *k = (const uint64_t *)keys;
#define SIMP_PLACE(Q, C)                                                                                            \
  SGNN_LAUNCH((k_simp_place<Q, C>), grid, dim3(256), 0, s, verts, nverts, faces, ntri, colors, order, start, csel, \
              nout, sel, k, origin, cell, out_verts, out_colors)
  if (quadric) {
    if (colors) SIMP_PLACE(true, true);
    else SIMP_PLACE(true, false);
  } else {
    if (colors) SIMP_PLACE(false, true);
    else SIMP_PLACE(false, false);
  }
#undef SIMP_PLACE
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
