// Depth frames tracked against a volume (sgnn_amd.track): the "frame to model" half that goes with the ray caster of
// raycast.hip.  The rules are listed in INTEGRATION.md section I; that text is the contract, and tests/track_ref.py
// restates it independently in NumPy.
//
// Kernels:
//   k_track_halve    one lane per output pixel of the next pyramid level (rule 9).
//   k_track_normals  one lane per pixel: the normal from the four axis neighbours (rule 10).
//   k_track_system   grid = (blocks over the live pixels, pairs).  A lane walks live pixels with a grid stride and
//                    keeps the 28 sums of rule 6 as fp64 accumulators and its pixel count; the pair record is
//                    wave-uniform and arrives by scalar loads.  Neighbouring live pixels associate to neighbouring
//                    model pixels, so the model gathers are nearly coalesced; no LDS staging.  A lane without an
//                    association adds zeros.  Reduction: csrc/gn_system.h, one 32-double partial per block.
//   k_gn_finish      one block per pair adds the partials in index order (csrc/gn_system.h).
// Tracking with colour (restated in tests/track_color_ref.py):
//   k_track_intensity        one lane per RGBA pixel (rule T1).
//   k_track_halve_intensity  one lane per output pixel: rule 9's selection applied to intensities (rule T2).
//   k_track_color_system     the photometric system of the pixels that pass rules 2-4 (rules T3-T5): the grid, the
//                            accumulators and the reduction of k_track_system, a bilinear sample of the model intensity
//                            as the residual.  track_associate() is rules 2-4 for both system kernels.
//
// The order of the additions is a function of (h, w) alone: no floating-point atomics, the same bits on every call.
//
// Built with -ffp-contract=off (Makefile): every product and sum is rounded on its own.
#include <math.h>
#include "common.h"
#include "gn_system.h"
#include "geom.h"

namespace {

constexpr int BLOCK = GN_BLOCK;

// rule 9
__global__ __launch_bounds__(BLOCK) void k_track_halve(const float *__restrict__ in, int total, int h, int w, int h2,
                                                      int w2, float delta, float *__restrict__ out) {
  const int idx = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
  if (idx >= total) return;
  const int i = idx % w2, t = idx / w2, j = t % h2, f = t / h2;
  const float *p = in + ((int64_t)f * h + 2 * j) * w + 2 * i;
  const float v[4] = {p[0], p[1], p[w], p[w + 1]};                    // raster order
  float c = INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (finite_f(v[k])) c = fminf(c, v[k]);
  float s = 0.f;
  int n = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (finite_f(v[k]) && v[k] - c <= delta) {
      s = s + v[k];
      ++n;
    }
  out[idx] = n ? __fdiv_rn(s, (float)n) : -INFINITY;
}

// rule 10
__global__ __launch_bounds__(BLOCK) void k_track_normals(const float *__restrict__ depth,
                                                        const float *__restrict__ intr, int total, int h, int w,
                                                        float delta, float *__restrict__ normal) {
  const int idx = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
  if (idx >= total) return;
  const int i = idx % w, t = idx / w, j = t % h, f = t / h;
  float n[3] = {NAN, NAN, NAN};
  if (i >= 1 && i + 1 < w && j >= 1 && j + 1 < h) {
    const float *p = depth + idx;
    const float dc = p[0], dl = p[-1], dr = p[1], du = p[-w], dd = p[w];
    if (finite_f(dc) && finite_f(dl) && finite_f(dr) && finite_f(du) && finite_f(dd) && fabsf(dl - dc) <= delta &&
        fabsf(dr - dc) <= delta && fabsf(du - dc) <= delta && fabsf(dd - dc) <= delta) {
      const float *K = intr + 4 * f;                // fx, fy, cx, cy
      const float xl = geom_unproject(K, 0, (float)(i - 1)), xc = geom_unproject(K, 0, (float)i);
      const float xr = geom_unproject(K, 0, (float)(i + 1));
      const float yu = geom_unproject(K, 1, (float)(j - 1)), yc = geom_unproject(K, 1, (float)j);
      const float yd = geom_unproject(K, 1, (float)(j + 1));
      // a = p(i+1, j) - p(i-1, j), b = p(i, j+1) - p(i, j-1)
      const float ax = xr * dr - xl * dl, ay = yc * dr - yc * dl, az = dr - dl;
      const float bx = xc * dd - xc * du, by = yd * dd - yu * du, bz = dd - du;
      geom_unit(by * az - bz * ay, bz * ax - bx * az, bx * ay - by * ax, n);   // b x a
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) normal[(int64_t)idx * 3 + c] = n[c];
}

// Rules 2-4 for one live pixel: what "passes the geometric gates" means, for both system kernels.
struct TrackHit {
  float q[3];      // the live point in the model camera (rule 2)
  float x, y;      // its unrounded model pixel (rule 3)
  float n[3];      // the model normal at the association
  float e[3];      // q - m (rule 4)
  int mi;          // v * wm + u, 0 without an association
};

template <bool ANGLE>
__device__ __forceinline__ bool track_associate(const sgnn_track_pair &P, bool pose_ok, float d, const float *l, int i,
                                                int j, const float *__restrict__ md, const float *__restrict__ mn,
                                                int hm, int wm, float max_dist2, float cos_min, TrackHit &H) {
  const float *T = P.t;
  const float Kl[4] = {P.intr_live[0], P.intr_live[1], P.intr_live[2], P.intr_live[3]};       // fx, fy, cx, cy
  const float Km[4] = {P.intr_model[0], P.intr_model[1], P.intr_model[2], P.intr_model[3]};
  // rule 2
  bool ok = pose_ok && finite_f(d) && d > 0.f;
  const float lx = geom_unproject(Kl, 0, (float)i) * d, ly = geom_unproject(Kl, 1, (float)j) * d;
  tsdf_affine(T, lx, ly, d, H.q);
  const float qx = H.q[0], qy = H.q[1], qz = H.q[2];
  // rule 3
  ok = ok && qz > 0.f;
  H.x = geom_project(Km, 0, qx, qz), H.y = geom_project(Km, 1, qy, qz);
  const float u = roundf(H.x), v = roundf(H.y);
  ok = ok && u >= 0.f && u < (float)wm && v >= 0.f && v < (float)hm;     // a NaN fails
  const int mi = ok ? (int)v * wm + (int)u : 0;
  H.mi = mi;
  const float dm = md[mi];
  const float nx = mn[(int64_t)mi * 3 + 0], ny = mn[(int64_t)mi * 3 + 1], nz = mn[(int64_t)mi * 3 + 2];
  H.n[0] = nx, H.n[1] = ny, H.n[2] = nz;
  ok = ok && finite_f(dm) && dm > 0.f && finite_f(nx) && finite_f(ny) && finite_f(nz);
  const float mx = geom_unproject(Km, 0, u) * dm, my = geom_unproject(Km, 1, v) * dm;
  // rule 4
  const float ex = qx - mx, ey = qy - my, ez = qz - dm;
  H.e[0] = ex, H.e[1] = ey, H.e[2] = ez;
  ok = ok && (ex * ex + ey * ey) + ez * ez <= max_dist2;
  if (ANGLE) {
    const float rx = geom_linear_row(T, 0, l[0], l[1], l[2]), ry = geom_linear_row(T, 1, l[0], l[1], l[2]);
    const float rz = geom_linear_row(T, 2, l[0], l[1], l[2]);
    ok = ok && (rx * nx + ry * ny) + rz * nz >= cos_min;                 // a NaN live normal fails
  }
  return ok;
}

template <bool ANGLE>
__global__ __launch_bounds__(BLOCK) void k_track_system(const float *__restrict__ depth,
                                                       const float *__restrict__ live_normal, int h, int w,
                                                       const float *__restrict__ model_depth,
                                                       const float *__restrict__ model_normal, int hm, int wm,
                                                       const sgnn_track_pair *__restrict__ pairs, float max_dist2,
                                                       float cos_min, double *__restrict__ ws,
                                                       float *__restrict__ residual, int32_t *__restrict__ assoc) {
  __shared__ double part[4][GN_ENTRIES];
  const int pair = (int)blockIdx.y;
  const sgnn_track_pair &P = pairs[pair];
  const bool pose_ok = P.t[0] == P.t[0];            // non-finite pose (the host stores NaN): an empty system
  const int npix = h * w;
  const int64_t live0 = (int64_t)pair * npix;
  const float *md = model_depth + (int64_t)pair * hm * wm;
  const float *mn = model_normal + (int64_t)pair * hm * wm * 3;
  double acc[GN_NSUM];
#pragma unroll
  for (int k = 0; k < GN_NSUM; ++k) acc[k] = 0.0;
  int count = 0;
  for (int px = (int)blockIdx.x * BLOCK + (int)threadIdx.x; px < npix; px += (int)gridDim.x * BLOCK) {
    const int j = px / w, i = px - j * w;
    TrackHit H;
    const bool ok = track_associate<ANGLE>(P, pose_ok, depth[live0 + px], ANGLE ? live_normal + (live0 + px) * 3 : nullptr,
                                           i, j, md, mn, hm, wm, max_dist2, cos_min, H);
    const float qx = H.q[0], qy = H.q[1], qz = H.q[2], nx = H.n[0], ny = H.n[1], nz = H.n[2];
    // rule 5
    const float r = (nx * H.e[0] + ny * H.e[1]) + nz * H.e[2];
    if (residual) residual[live0 + px] = ok ? r : NAN;
    if (assoc) assoc[live0 + px] = ok ? H.mi : -1;
    float J[7];
    J[0] = ok ? qy * nz - qz * ny : 0.f;
    J[1] = ok ? qz * nx - qx * nz : 0.f;
    J[2] = ok ? qx * ny - qy * nx : 0.f;
    J[3] = ok ? nx : 0.f;
    J[4] = ok ? ny : 0.f;
    J[5] = ok ? nz : 0.f;
    J[6] = ok ? r : 0.f;
    gn_accumulate(acc, J);                          // rule 6: exact products, fp64 sums
    count += ok ? 1 : 0;
  }
  gn_block_reduce(acc, count, part, ws + ((int64_t)pair * gridDim.x + blockIdx.x) * GN_ENTRIES);
}

// section T rule T1
__global__ __launch_bounds__(BLOCK) void k_track_intensity(const uint8_t *__restrict__ rgba, int total,
                                                          float *__restrict__ out) {
  const int idx = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
  if (idx >= total) return;
  const uchar4 c = reinterpret_cast<const uchar4 *>(rgba)[idx];
  const int y = 77 * (int)c.x + 150 * (int)c.y + 29 * (int)c.z;
  out[idx] = c.w ? __fdiv_rn((float)y, 256.f) : NAN;                  // exact: y < 2^16
}

// rule T2: rule 9's selection of the block's pixels, applied to their intensities
__global__ __launch_bounds__(BLOCK) void k_track_halve_intensity(const float *__restrict__ depth,
                                                                const float *__restrict__ in, int total, int h, int w,
                                                                int h2, int w2, float delta, float *__restrict__ out) {
  const int idx = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
  if (idx >= total) return;
  const int i = idx % w2, t = idx / w2, j = t % h2, f = t / h2;
  const int64_t at = ((int64_t)f * h + 2 * j) * w + 2 * i;
  const float *p = depth + at, *c4 = in + at;
  const float v[4] = {p[0], p[1], p[w], p[w + 1]};                    // raster order
  const float y[4] = {c4[0], c4[1], c4[w], c4[w + 1]};
  float c = INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (finite_f(v[k])) c = fminf(c, v[k]);
  float s = 0.f;
  int n = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (finite_f(v[k]) && v[k] - c <= delta && y[k] == y[k]) {
      s = s + y[k];
      ++n;
    }
  out[idx] = n ? __fdiv_rn(s, (float)n) : NAN;
}

// rules T3-T5: the photometric system of the pixels that pass rules 2-4; a kernel of its own next to k_track_system
template <bool ANGLE>
__global__ __launch_bounds__(BLOCK) void k_track_color_system(
    const float *__restrict__ depth, const float *__restrict__ live_normal, const float *__restrict__ live_intensity,
    int h, int w, const float *__restrict__ model_depth, const float *__restrict__ model_normal,
    const float *__restrict__ model_intensity, int hm, int wm, const sgnn_track_pair *__restrict__ pairs,
    float max_dist2, float cos_min, float max_dist, float max_intensity, double *__restrict__ ws,
    float *__restrict__ residual, int32_t *__restrict__ cell) {
  __shared__ double part[4][GN_ENTRIES];
  const int pair = (int)blockIdx.y;
  const sgnn_track_pair &P = pairs[pair];
  const bool pose_ok = P.t[0] == P.t[0];
  const float fxm = P.intr_model[0], fym = P.intr_model[1];
  const int npix = h * w;
  const int64_t live0 = (int64_t)pair * npix;
  const float *md = model_depth + (int64_t)pair * hm * wm;
  const float *mn = model_normal + (int64_t)pair * hm * wm * 3;
  const float *mc = model_intensity + (int64_t)pair * hm * wm;
  double acc[GN_NSUM];
#pragma unroll
  for (int k = 0; k < GN_NSUM; ++k) acc[k] = 0.0;
  int count = 0;
  for (int px = (int)blockIdx.x * BLOCK + (int)threadIdx.x; px < npix; px += (int)gridDim.x * BLOCK) {
    const int j = px / w, i = px - j * w;
    TrackHit H;
    bool ok = track_associate<ANGLE>(P, pose_ok, depth[live0 + px], ANGLE ? live_normal + (live0 + px) * 3 : nullptr, i,
                                     j, md, mn, hm, wm, max_dist2, cos_min, H);
    const float qx = H.q[0], qy = H.q[1], qz = H.q[2];
    // rule T3
    const float il = live_intensity[live0 + px];
    ok = ok && il == il;
    const float x0 = floorf(H.x), y0 = floorf(H.y);
    const float a = H.x - x0, b = H.y - y0;
    ok = ok && x0 >= 0.f && x0 + 1.f < (float)wm && y0 >= 0.f && y0 + 1.f < (float)hm;   // a NaN fails
    const int c00 = ok ? (int)y0 * wm + (int)x0 : 0;
    const int c10 = ok ? c00 + 1 : 0, c01 = ok ? c00 + wm : 0, c11 = ok ? c00 + wm + 1 : 0;   // never read outside
    const float i00 = mc[c00], i10 = mc[c10], i01 = mc[c01], i11 = mc[c11];
    const float d00 = md[c00], d10 = md[c10], d01 = md[c01], d11 = md[c11];
    ok = ok && i00 == i00 && i10 == i10 && i01 == i01 && i11 == i11;
    ok = ok && finite_f(d00) && finite_f(d10) && finite_f(d01) && finite_f(d11);
    ok = ok && fabsf(d00 - qz) <= max_dist && fabsf(d10 - qz) <= max_dist && fabsf(d01 - qz) <= max_dist &&
         fabsf(d11 - qz) <= max_dist;
    // rule T4
    const float oma = 1.f - a, omb = 1.f - b;
    const float im = (i00 * oma + i10 * a) * omb + (i01 * oma + i11 * a) * b;
    const float gx = (i10 - i00) * omb + (i11 - i01) * b;
    const float gy = (i01 - i00) * oma + (i11 - i10) * a;
    const float r = im - il;
    ok = ok && fabsf(r) <= max_intensity;
    const float kx = __fdiv_rn(gx * fxm, qz), ky = __fdiv_rn(gy * fym, qz);
    const float kz = -__fdiv_rn(kx * qx + ky * qy, qz);
    if (residual) residual[live0 + px] = ok ? r : NAN;
    if (cell) cell[live0 + px] = ok ? c00 : -1;
    float J[7];
    J[0] = ok ? qy * kz - qz * ky : 0.f;
    J[1] = ok ? qz * kx - qx * kz : 0.f;
    J[2] = ok ? qx * ky - qy * kx : 0.f;
    J[3] = ok ? kx : 0.f;
    J[4] = ok ? ky : 0.f;
    J[5] = ok ? kz : 0.f;
    J[6] = ok ? r : 0.f;
    gn_accumulate(acc, J);                          // rule T5: the sums of rule 6
    count += ok ? 1 : 0;
  }
  gn_block_reduce(acc, count, part, ws + ((int64_t)pair * gridDim.x + blockIdx.x) * GN_ENTRIES);
}

}  // namespace

SGNN_EXPORT int sgnn_track_halve(const float *depth, int nframes, int h, int w, float delta, float *out,
                                 sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nframes >= 0 && h >= 1 && w >= 1 && (int64_t)nframes * h * w < ((int64_t)1 << 31));
  SGNN_CHECK_ARG(delta > 0.f);
  const int h2 = h / 2, w2 = w / 2;
  const int64_t total = (int64_t)nframes * h2 * w2;
  if (total == 0) return SGNN_OK;
  SGNN_CHECK_ARG(depth && out);
  SGNN_LAUNCH(k_track_halve, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, depth,
              (int)total, h, w, h2, w2, delta, out);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_track_normals(const float *depth, const float *intr, int nframes, int h, int w, float delta,
                                   float *normal, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nframes >= 0 && h >= 1 && w >= 1 && (int64_t)nframes * h * w < ((int64_t)1 << 31));
  SGNN_CHECK_ARG(delta > 0.f);
  const int64_t total = (int64_t)nframes * h * w;
  if (total == 0) return SGNN_OK;
  SGNN_CHECK_ARG(depth && intr && normal);
  SGNN_LAUNCH(k_track_normals, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream,
              depth, intr, (int)total, h, w, delta, normal);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_track_system(const float *depth, const float *live_normal, int h, int w, const float *model_depth,
                                  const float *model_normal, int hm, int wm, const sgnn_track_pair *pairs, int npairs,
                                  float max_dist2, float cos_min, double *out, float *residual, int32_t *assoc,
                                  void *ws, int64_t ws_bytes, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(npairs >= 0 && npairs <= 65535 && h >= 1 && w >= 1 && hm >= 1 && wm >= 1);
  SGNN_CHECK_ARG((int64_t)npairs * h * w < ((int64_t)1 << 31) && (int64_t)npairs * hm * wm < ((int64_t)1 << 31));
  SGNN_CHECK_ARG((int64_t)h * w < ((int64_t)1 << 31) - (int64_t)SGNN_TRACK_MAX_BLOCKS * BLOCK);   // the stride loop's index
  SGNN_CHECK_ARG(max_dist2 > 0.f);
  if (npairs == 0) return SGNN_OK;
  SGNN_CHECK_ARG(depth && model_depth && model_normal && pairs && out && ws);
  hipStream_t s = (hipStream_t)stream;
  return gn_launch((int64_t)h * w, SGNN_TRACK_MAX_BLOCKS, npairs, ws, ws_bytes, out, s, [&](int nblk) {
    const dim3 grid(nblk, npairs);
    if (live_normal)
      SGNN_LAUNCH((k_track_system<true>), grid, dim3(BLOCK), 0, s, depth, live_normal, h, w, model_depth, model_normal,
                  hm, wm, pairs, max_dist2, cos_min, (double *)ws, residual, assoc);
    else
      SGNN_LAUNCH((k_track_system<false>), grid, dim3(BLOCK), 0, s, depth, live_normal, h, w, model_depth, model_normal,
                  hm, wm, pairs, max_dist2, cos_min, (double *)ws, residual, assoc);
  });
}

SGNN_EXPORT int sgnn_track_intensity(const uint8_t *rgba, int64_t n, float *out, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31) - BLOCK);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(rgba && out);
  SGNN_LAUNCH(k_track_intensity, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, rgba,
              (int)n, out);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_track_halve_intensity(const float *depth, const float *intensity, int nframes, int h, int w,
                                           float delta, float *out, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nframes >= 0 && h >= 1 && w >= 1 && (int64_t)nframes * h * w < ((int64_t)1 << 31));
  SGNN_CHECK_ARG(delta > 0.f);
  const int h2 = h / 2, w2 = w / 2;
  const int64_t total = (int64_t)nframes * h2 * w2;
  if (total == 0) return SGNN_OK;
  SGNN_CHECK_ARG(depth && intensity && out);
  SGNN_LAUNCH(k_track_halve_intensity, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0,
              (hipStream_t)stream, depth, intensity, (int)total, h, w, h2, w2, delta, out);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_track_color_system(const float *depth, const float *live_normal, const float *live_intensity,
                                        int h, int w, const float *model_depth, const float *model_normal,
                                        const float *model_intensity, int hm, int wm, const sgnn_track_pair *pairs,
                                        int npairs, float max_dist2, float cos_min, float max_dist,
                                        float max_intensity, double *out, float *residual, int32_t *cell, void *ws,
                                        int64_t ws_bytes, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(npairs >= 0 && npairs <= 65535 && h >= 1 && w >= 1 && hm >= 1 && wm >= 1);
  SGNN_CHECK_ARG((int64_t)npairs * h * w < ((int64_t)1 << 31) && (int64_t)npairs * hm * wm < ((int64_t)1 << 31));
  SGNN_CHECK_ARG((int64_t)h * w < ((int64_t)1 << 31) - (int64_t)SGNN_TRACK_MAX_BLOCKS * BLOCK);   // the stride loop's index
  SGNN_CHECK_ARG(max_dist2 > 0.f && max_dist > 0.f && max_intensity > 0.f);
  if (npairs == 0) return SGNN_OK;
  SGNN_CHECK_ARG(depth && live_intensity && model_depth && model_normal && model_intensity && pairs && out && ws);
  hipStream_t s = (hipStream_t)stream;
  return gn_launch((int64_t)h * w, SGNN_TRACK_MAX_BLOCKS, npairs, ws, ws_bytes, out, s, [&](int nblk) {
    const dim3 grid(nblk, npairs);
    if (live_normal)
      SGNN_LAUNCH((k_track_color_system<true>), grid, dim3(BLOCK), 0, s, depth, live_normal, live_intensity, h, w,
                  model_depth, model_normal, model_intensity, hm, wm, pairs, max_dist2, cos_min, max_dist,
                  max_intensity, (double *)ws, residual, cell);
    else
      SGNN_LAUNCH((k_track_color_system<false>), grid, dim3(BLOCK), 0, s, depth, live_normal, live_intensity, h, w,
                  model_depth, model_normal, model_intensity, hm, wm, pairs, max_dist2, cos_min, max_dist,
                  max_intensity, (double *)ws, residual, cell);
  });
}
