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
//
// The order of the additions is a function of (h, w) alone: no floating-point atomics, the same bits on every call.
//
// Built with -ffp-contract=off (Makefile): every product and sum is rounded on its own.
#include <math.h>
#include "common.h"
#include "gn_system.h"
#include "tsdf.h"

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
  float nx = NAN, ny = NAN, nz = NAN;
  if (i >= 1 && i + 1 < w && j >= 1 && j + 1 < h) {
    const float *p = depth + idx;
    const float dc = p[0], dl = p[-1], dr = p[1], du = p[-w], dd = p[w];
    if (finite_f(dc) && finite_f(dl) && finite_f(dr) && finite_f(du) && finite_f(dd) && fabsf(dl - dc) <= delta &&
        fabsf(dr - dc) <= delta && fabsf(du - dc) <= delta && fabsf(dd - dc) <= delta) {
      const float fx = intr[4 * f + 0], fy = intr[4 * f + 1], cx = intr[4 * f + 2], cy = intr[4 * f + 3];
      const float xl = __fdiv_rn((float)(i - 1) - cx, fx), xc = __fdiv_rn((float)i - cx, fx);
      const float xr = __fdiv_rn((float)(i + 1) - cx, fx);
      const float yu = __fdiv_rn((float)(j - 1) - cy, fy), yc = __fdiv_rn((float)j - cy, fy);
      const float yd = __fdiv_rn((float)(j + 1) - cy, fy);
      // a = p(i+1, j) - p(i-1, j), b = p(i, j+1) - p(i, j-1)
      const float ax = xr * dr - xl * dl, ay = yc * dr - yc * dl, az = dr - dl;
      const float bx = xc * dd - xc * du, by = yd * dd - yu * du, bz = dd - du;
      const float qx = by * az - bz * ay, qy = bz * ax - bx * az, qz = bx * ay - by * ax;   // b x a
      const float len = (float)sqrt((double)((qx * qx + qy * qy) + qz * qz));              // correctly rounded
      if (len > 0.f && len < INFINITY) {
        nx = __fdiv_rn(qx, len);
        ny = __fdiv_rn(qy, len);
        nz = __fdiv_rn(qz, len);
      }
    }
  }
  normal[(int64_t)idx * 3 + 0] = nx;
  normal[(int64_t)idx * 3 + 1] = ny;
  normal[(int64_t)idx * 3 + 2] = nz;
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
  const float *T = P.t;
  const bool pose_ok = T[0] == T[0];                // non-finite pose (the host stores NaN): an empty system
  const float fxl = P.intr_live[0], fyl = P.intr_live[1], cxl = P.intr_live[2], cyl = P.intr_live[3];
  const float fxm = P.intr_model[0], fym = P.intr_model[1], cxm = P.intr_model[2], cym = P.intr_model[3];
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
    // rule 2
    const float d = depth[live0 + px];
    bool ok = pose_ok && finite_f(d) && d > 0.f;
    const float lx = __fdiv_rn((float)i - cxl, fxl) * d, ly = __fdiv_rn((float)j - cyl, fyl) * d;
    float q[3];
    tsdf_affine(T, lx, ly, d, q);
    const float qx = q[0], qy = q[1], qz = q[2];
    // rule 3
    ok = ok && qz > 0.f;
    const float u = roundf(__fdiv_rn(qx * fxm, qz) + cxm), v = roundf(__fdiv_rn(qy * fym, qz) + cym);
    ok = ok && u >= 0.f && u < (float)wm && v >= 0.f && v < (float)hm;     // a NaN fails
    const int mi = ok ? (int)v * wm + (int)u : 0;
    const float dm = md[mi];
    const float nx = mn[(int64_t)mi * 3 + 0], ny = mn[(int64_t)mi * 3 + 1], nz = mn[(int64_t)mi * 3 + 2];
    ok = ok && finite_f(dm) && dm > 0.f && finite_f(nx) && finite_f(ny) && finite_f(nz);
    const float mx = __fdiv_rn(u - cxm, fxm) * dm, my = __fdiv_rn(v - cym, fym) * dm;
    // rule 4
    const float ex = qx - mx, ey = qy - my, ez = qz - dm;
    ok = ok && (ex * ex + ey * ey) + ez * ez <= max_dist2;
    if (ANGLE) {
      const float *l = live_normal + (live0 + px) * 3;
      const float l0 = l[0], l1 = l[1], l2 = l[2];
      const float rx = (T[0] * l0 + T[1] * l1) + T[2] * l2;
      const float ry = (T[4] * l0 + T[5] * l1) + T[6] * l2;
      const float rz = (T[8] * l0 + T[9] * l1) + T[10] * l2;
      ok = ok && (rx * nx + ry * ny) + rz * nz >= cos_min;                 // a NaN live normal fails
    }
    // rule 5
    const float r = (nx * ex + ny * ey) + nz * ez;
    if (residual) residual[live0 + px] = ok ? r : NAN;
    if (assoc) assoc[live0 + px] = ok ? mi : -1;
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
