// Mesh tables shared by marching cubes' clean-up, the component filter and the simplifier (include/sgnn_hip.h, "shared
// mesh tables"): numbering of selected rows, the remap + degenerate / duplicate face filter, row gathers of (., 3) arrays
// and the size of a first-member table.  Integer-only.
#include "common.h"
#include "first_table.h"

SGNN_EXPORT int64_t sgnn_weld_slots(int64_t n) { return n < 8 ? 16 : 2 * n + 1; }

// faces: remap through the weld or the clustering, drop degenerate (marching_cubes.cpp:298-321) and duplicate (:266-297)
// triangles.  A face's key is its sorted vertex triple.
__device__ __forceinline__ Key3 tri_sorted(const int32_t *__restrict__ f) {
  int a = f[0], b = f[1], c = f[2], t;
  if (a > b) { t = a; a = b; b = t; }
  if (b > c) { t = b; b = c; c = t; }
  if (a > b) { t = a; a = b; b = t; }
  return Key3{a, b, c};
}

// newid[sel[p]] = p : new index of every creator vertex (cnt order of :405-410 = soup order)
__global__ __launch_bounds__(256) void k_weld_number(const int32_t *__restrict__ sel, int64_t n, int32_t *__restrict__ newid) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < n) newid[sel[p]] = (int32_t)p;
}

__global__ __launch_bounds__(256) void k_faces_remap(const int32_t *__restrict__ creator_of,
                                                    const int32_t *__restrict__ newid, int64_t ntri,
                                                    int32_t *__restrict__ faces) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < 3 * ntri) faces[e] = newid[creator_of[e]];
}

__device__ __forceinline__ bool tri_degenerate(const int32_t *__restrict__ f) {
  return f[0] == f[1] || f[0] == f[2] || f[1] == f[2];
}

// set of unordered vertex triples (first_table.h): frep[slot] = some face of the triple, ffirst[slot] = its first face;
// degenerate faces never enter it (:440 runs first)
__global__ __launch_bounds__(256) void k_faces_insert(const int32_t *__restrict__ faces, int64_t ntri,
                                                     int32_t *__restrict__ frep, int32_t *__restrict__ ffirst,
                                                     int64_t cap) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= ntri || tri_degenerate(faces + 3 * t)) return;
  const Key3 key = tri_sorted(faces + 3 * t);
  first_insert(frep, ffirst, cap, (int64_t)(weld_hash(key) % (uint64_t)cap), (int32_t)t, (int32_t)t,
               [&](int32_t u) { return tri_sorted(faces + 3 * (int64_t)u) == key; });
}

// keep[t] = non-degenerate and the first face of its (unordered) vertex triple
__global__ __launch_bounds__(256) void k_faces_keep(const int32_t *__restrict__ faces, int64_t ntri,
                                                   const int32_t *__restrict__ frep, const int32_t *__restrict__ ffirst,
                                                   int64_t cap, uint8_t *__restrict__ keep) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= ntri) return;
  if (tri_degenerate(faces + 3 * t)) {
    keep[t] = 0;
    return;
  }
  const Key3 key = tri_sorted(faces + 3 * t);      // present: k_faces_insert ran first, same stream and faces
  const int64_t h = first_find<true>(frep, cap, (int64_t)(weld_hash(key) % (uint64_t)cap),
                                     [&](int32_t u) { return tri_sorted(faces + 3 * (int64_t)u) == key; });
  keep[t] = ffirst[h] == (int32_t)t;
}

SGNN_EXPORT int sgnn_weld_number(const int32_t *sel, int64_t n, int32_t *newid, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(sel && newid);
  SGNN_LAUNCH(k_weld_number, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sel, n, newid);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_mesh_faces(const int32_t *creator_of, const int32_t *newid, int64_t ntri, int32_t *faces,
                                int32_t *frep, int32_t *ffirst, int64_t cap, uint8_t *keep, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(ntri >= 0 && cap >= sgnn_weld_slots(ntri) && frep && ffirst);
  hipStream_t s = (hipStream_t)stream;
  SGNN_HIP_TRY(hipMemsetAsync(frep, 0xFF, (size_t)cap * sizeof(int32_t), s));
  SGNN_HIP_TRY(hipMemsetAsync(ffirst, 0x7F, (size_t)cap * sizeof(int32_t), s));
  if (ntri == 0) return SGNN_OK;
  SGNN_CHECK_ARG(creator_of && newid && faces && keep);
  const dim3 grid((unsigned)((ntri + 255) / 256));
  SGNN_LAUNCH(k_faces_remap, dim3((unsigned)((3 * ntri + 255) / 256)), dim3(256), 0, s, creator_of, newid, ntri,
                     faces);
  SGNN_LAUNCH(k_faces_insert, grid, dim3(256), 0, s, (const int32_t *)faces, ntri, frep, ffirst, cap);
  SGNN_LAUNCH(k_faces_keep, grid, dim3(256), 0, s, (const int32_t *)faces, ntri, (const int32_t *)frep,
                     (const int32_t *)ffirst, cap, keep);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

// out rows p < n: rows sel[p] of a (., 3) float / uint8 / int32 array
template <typename T>
__global__ __launch_bounds__(256) void k_take3(const T *__restrict__ src, const int32_t *__restrict__ sel, int64_t n,
                                              T *__restrict__ dst) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= 3 * n) return;
  dst[e] = src[3 * (int64_t)sel[e / 3] + e % 3];
}

SGNN_EXPORT int sgnn_take_rows3(const void *src, int elem_bytes, const int32_t *sel, int64_t n, void *dst,
                                sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && (elem_bytes == 1 || elem_bytes == 4));
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(src && sel && dst);
  const dim3 grid((unsigned)((3 * n + 255) / 256));
  if (elem_bytes == 4)
    SGNN_LAUNCH((k_take3<uint32_t>), grid, dim3(256), 0, (hipStream_t)stream, (const uint32_t *)src, sel, n,
                       (uint32_t *)dst);
  else
    SGNN_LAUNCH((k_take3<uint8_t>), grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t *)src, sel, n,
                       (uint8_t *)dst);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
