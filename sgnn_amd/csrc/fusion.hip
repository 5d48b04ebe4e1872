// TSDF fusion of depth frames into a scan volume (SG-NN's data generation: datagen/GenerateScans, the step before the
// .sdf / .knw files that io.hip reads).  The rules restated here are listed in INTEGRATION.md "TSDF fusion"; the
// reference's Fuser / VoxelGrid / CameraUtil depend on a library that is not part of this project, so those rules are
// the contract, and tests/fusion_ref.py restates them independently in NumPy.
//
// Kernels:
//   k_fuse_depth_raw      uint16 frames -> metric fp32 depth (nearest-index resampling, range test)     1 thread / pixel
//   k_fuse_bilateral      edge-preserving filter of the metric frames                                   1 thread / pixel
//   k_fuse_integrate      the hot path: every voxel folds a chunk of frames in input order, its (sdf, weight, free
//                         counter) in registers; state is read and written once per chunk
//   k_fuse_flag           |sdf| <= keep (the sparse file filter), optionally |sdf/vs| < truncation and z < max_z
//   k_fuse_emit_block     kept voxels -> (x,y,z) u32 + metric sdf f32, the .sdf block layout
//   k_fuse_emit_rows      kept voxels -> [z,y,x,0] int64 rows + sdf/vs features (the collated scene input)
//   k_fuse_known          u8 known codes of the .knw file
// Compaction between flag and emit is sgnn_compact_mask (stable: raster order, x fastest).
//
// Built with -ffp-contract=off (Makefile): every product and sum below is rounded on its own, so the fp32
// restatement in the tests reproduces sdf, weight and free counter bit for bit.
#include <math.h>
#include "common.h"

namespace {

// workgroup brick of the integration: 64 x 4 x 1 voxels, x contiguous (state loads / stores coalesce)
constexpr int BRICK_X = 64, BRICK_Y = 4;

struct FuseObb {
  int on;
  float a[3];      // corner
  float e[3][3];   // edge vectors
  float ee[3];     // dot(e_k, e_k), formed on the host in the same order as below
};

__device__ __forceinline__ bool box_hits_brick(const int32_t *b, int x0, int x1, int y0, int y1, int k) {
  return b[0] <= x1 && b[1] >= x0 && b[2] <= y1 && b[3] >= y0 && b[4] <= k && b[5] >= k;
}

// 0 <= dot(q - a, e_k) <= dot(e_k, e_k) for k = 0, 1, 2; dot in the order (x*x' + y*y') + z*z'
__device__ __forceinline__ bool obb_contains(const FuseObb &o, float qx, float qy, float qz) {
  const float rx = qx - o.a[0], ry = qy - o.a[1], rz = qz - o.a[2];
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float d = (rx * o.e[k][0] + ry * o.e[k][1]) + rz * o.e[k][2];
    in = in && d >= 0.f && d <= o.ee[k];
  }
  return in;
}

__global__ __launch_bounds__(256) void k_fuse_depth_raw(const uint16_t *__restrict__ raw, int64_t npix, int hr, int wr,
                                                       int h, int w, float inv_shift, float min_depth, float max_depth,
                                                       float *__restrict__ out) {
  const float fx = __fdiv_rn((float)(wr - 1), (float)(w - 1));
  const float fy = __fdiv_rn((float)(hr - 1), (float)(h - 1));
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += stride) {
    const int64_t f = p / ((int64_t)h * w);
    const int r = (int)(p - f * h * w);
    const int j = r / w, i = r - j * w;
    int x = (int)roundf((float)i * fx), y = (int)roundf((float)j * fy);   // half away from zero, as std::round
    x = min(x, wr - 1);                                                    // never taken: (w-1)*fx rounds to wr-1
    y = min(y, hr - 1);
    const uint16_t d = raw[(f * hr + y) * wr + x];
    const float fd = inv_shift * (float)d;
    out[p] = (d == 0 || fd < min_depth || fd > max_depth) ? -INFINITY : fd;
  }
}

// output = sum w * d / sum w over finite neighbours within `radius`, w = exp(-(dx^2+dy^2) / (2 sd^2)) *
// exp(-(d - c)^2 / (2 sr^2)); -inf where the centre is not finite or the weights sum to 0
__global__ __launch_bounds__(256) void k_fuse_bilateral(const float *__restrict__ in, int64_t npix, int h, int w,
                                                       int radius, float two_sd2, float two_sr2,
                                                       float *__restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += stride) {
    const int64_t f = p / ((int64_t)h * w);
    const int r = (int)(p - f * h * w);
    const int y = r / w, x = r - y * w;
    const float *img = in + f * h * w;
    const float c = img[r];
    float res = -INFINITY;
    if (isfinite(c)) {
      float sum = 0.f, sumw = 0.f;
      for (int m = max(x - radius, 0); m <= min(x + radius, w - 1); ++m) {
        for (int n = max(y - radius, 0); n <= min(y + radius, h - 1); ++n) {
          const float d = img[n * w + m];
          if (!isfinite(d)) continue;
          const int ddx = m - x, ddy = n - y;
          const float diff = d - c;
          const float wt = expf(-__fdiv_rn((float)(ddx * ddx + ddy * ddy), two_sd2)) *
                           expf(-__fdiv_rn(diff * diff, two_sr2));
          sumw += wt;
          sum += wt * d;
        }
      }
      if (sumw > 0.f) res = __fdiv_rn(sum, sumw);
    }
    out[p] = res;
  }
}

// Frames f0 .. f1-1 into the volume.  Workgroup = one 64x4x1 brick; the frame loop is workgroup-uniform (the table
// is read with scalar loads, the brick test needs no lane), so a frame whose box misses the brick costs a few
// scalar instructions and a brick that no frame of the chunk touches neither loads nor stores its state.
__global__ __launch_bounds__(256) void k_fuse_integrate(float *__restrict__ sdf, uint8_t *__restrict__ weight,
                                                       int32_t *__restrict__ freec, int dx, int dy,
                                                       const float *__restrict__ depth, int h, int w,
                                                       const sgnn_fuse_frame *__restrict__ fr, int f0, int f1,
                                                       float vs, float dmin, float dmax, FuseObb obb) {
  const int x0 = blockIdx.x * BRICK_X, y0 = blockIdx.y * BRICK_Y, k = blockIdx.z;
  const int x1 = min(x0 + BRICK_X - 1, dx - 1), y1 = min(y0 + BRICK_Y - 1, dy - 1);
  bool any = false;
  for (int f = f0; f < f1 && !any; ++f) any = box_hits_brick(fr[f].box, x0, x1, y0, y1, k);
  if (!any) return;

  const int i = x0 + (int)(threadIdx.x & (BRICK_X - 1)), j = y0 + (int)(threadIdx.x / BRICK_X);
  const bool inside = i < dx && j < dy;
  const int64_t v = ((int64_t)k * dy + j) * dx + i;
  float s = -INFINITY;
  int wt = 0;
  int32_t fc = 0;
  if (inside) {
    s = sdf[v];
    wt = weight[v];
    fc = freec[v];
  }
  const float fi = (float)i, fj = (float)j, fk = (float)k;
  const bool eligible = inside && (!obb.on || obb_contains(obb, fi, fj, fk));
  const uint32_t frame_bytes = (uint32_t)h * (uint32_t)w * 4u;
  const float trunc0 = vs * 3.0f;

  for (int f = f0; f < f1; ++f) {
    const sgnn_fuse_frame &F = fr[f];
    if (!box_hits_brick(F.box, x0, x1, y0, y1, k)) continue;
    const bool inbox = eligible && i >= F.box[0] && i <= F.box[1] && j >= F.box[2] && j <= F.box[3];
    const float *m = F.m;
    const float px3 = ((m[0] * fi + m[1] * fj) + m[2] * fk) + m[3];
    const float py3 = ((m[4] * fi + m[5] * fj) + m[6] * fk) + m[7];
    const float pz = ((m[8] * fi + m[9] * fj) + m[10] * fk) + m[11];
    const float px = __fdiv_rn(px3 * F.intr[0], pz) + F.intr[2];
    const float py = __fdiv_rn(py3 * F.intr[1], pz) + F.intr[3];
    const float rx = roundf(px), ry = roundf(py);                        // NaN / inf fail both range tests
    const bool on_image = inbox && rx >= 0.f && rx < (float)w && ry >= 0.f && ry < (float)h;
    // pixels off the image read at an out-of-range offset: the buffer load returns 0, which fails the range test
    const uint32_t off = on_image ? ((uint32_t)ry * (uint32_t)w + (uint32_t)rx) * 4u : 0xFFFFFFFFu;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(depth + F.offset), 0, (int)frame_bytes, 0x00020000);
    const float d = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
    if (!(on_image && d >= dmin && d <= dmax)) continue;
    if (pz < d) ++fc;                                                     // voxel in front of the observation
    float sd = d - pz;
    const float trunc = trunc0 + d * vs;
    if (!(sd > -trunc)) continue;
    sd = sd >= 0.f ? fminf(trunc, sd) : fmaxf(-trunc, sd);
    const float z01 = __fdiv_rn(d - 0.4f, 4.0f - 0.4f);                 // the weight ramp is fixed to 0.4 .. 4.0 m
    const float wu = fmaxf(4.5f * (1.0f - z01), 1.0f);
    if (s == -INFINITY) s = sd;
    else s = __fdiv_rn(s * (float)wt + sd * wu, (float)wt + wu);
    wt = min(wt + (int)wu, 255);
  }
  if (inside) {
    sdf[v] = s;
    weight[v] = (uint8_t)wt;
    freec[v] = fc;
  }
}

__global__ __launch_bounds__(256) void k_fuse_flag(const float *__restrict__ sdf, int64_t n, int64_t plane,
                                                  float keep_abs, float truncation, float vs, int64_t max_z,
                                                  uint8_t *__restrict__ mask) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += stride) {
    const float s = sdf[v];
    bool keep = fabsf(s) <= keep_abs;
    if (truncation > 0.f) keep = keep && fabsf(__fdiv_rn(s, vs)) < truncation && v / plane < max_z;
    mask[v] = keep;
  }
}

__global__ __launch_bounds__(256) void k_fuse_emit_block(const float *__restrict__ sdf, int dx, int dy,
                                                        const int32_t *__restrict__ sel,
                                                        const int64_t *__restrict__ count,
                                                        uint32_t *__restrict__ locs_xyz, float *__restrict__ vals) {
  const int64_t m = *count;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < m; q += stride) {
    const int64_t v = sel[q];
    const int64_t row = v / dx;
    locs_xyz[3 * q] = (uint32_t)(v - row * dx);
    locs_xyz[3 * q + 1] = (uint32_t)(row % dy);
    locs_xyz[3 * q + 2] = (uint32_t)(row / dy);
    vals[q] = sdf[v];
  }
}

__global__ __launch_bounds__(256) void k_fuse_emit_rows(const float *__restrict__ sdf, int dx, int dy, float vs,
                                                       const int32_t *__restrict__ sel,
                                                       const int64_t *__restrict__ count,
                                                       int64_t *__restrict__ locs, float *__restrict__ feats) {
  const int64_t m = *count;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < m; q += stride) {
    const int64_t v = sel[q];
    const int64_t row = v / dx;
    longlong2 *o = reinterpret_cast<longlong2 *>(locs + 4 * q);
    o[0] = make_longlong2((long long)(row / dy), (long long)(row % dy));
    o[1] = make_longlong2((long long)(v - row * dx), 0ll);
    feats[q] = __fdiv_rn(sdf[v], vs);
  }
}

__global__ __launch_bounds__(256) void k_fuse_known(const float *__restrict__ sdf, int64_t n, float vs,
                                                   uint8_t *__restrict__ known) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += stride) {
    known[v] = sgnn_known_code(sdf[v], vs);
  }
}

}  // namespace

SGNN_EXPORT int sgnn_fuse_depth_raw(const uint16_t *raw, int nframes, int h_raw, int w_raw, int h, int w,
                                    float depth_shift, float min_depth, float max_depth, float *out,
                                    sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nframes >= 0 && h_raw >= 2 && w_raw >= 2 && h >= 2 && w >= 2 && depth_shift > 0.f);
  if (nframes == 0) return SGNN_OK;
  SGNN_CHECK_ARG(raw && out);
  const int64_t npix = (int64_t)nframes * h * w;
  SGNN_LAUNCH(k_fuse_depth_raw, dim3(sgnn_grid_for(npix, 256, 8192)), dim3(256), 0, (hipStream_t)stream, raw, npix,
              h_raw, w_raw, h, w, 1.0f / depth_shift, min_depth, max_depth, out);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_fuse_bilateral(const float *in, int nframes, int h, int w, float sigma_d, float sigma_r, float *out,
                                    sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nframes >= 0 && h >= 1 && w >= 1 && sigma_d > 0.f && sigma_r > 0.f && sigma_d <= 64.f);
  if (nframes == 0) return SGNN_OK;
  SGNN_CHECK_ARG(in && out && in != out);
  const int64_t npix = (int64_t)nframes * h * w;
  const int radius = (int)ceil(2.0 * (double)sigma_d);
  SGNN_LAUNCH(k_fuse_bilateral, dim3(sgnn_grid_for(npix, 256, 8192)), dim3(256), 0, (hipStream_t)stream, in, npix, h,
              w, radius, 2.0f * sigma_d * sigma_d, 2.0f * sigma_r * sigma_r, out);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_fuse_integrate(float *sdf, uint8_t *weight, int32_t *free_ctr, int dx, int dy, int dz,
                                    const float *depth, int h, int w, const sgnn_fuse_frame *frames, int nframes,
                                    int chunk, float voxel_size, float depth_min, float depth_max, const float *obb,
                                    sgnn_stream_t stream) {
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && dz >= 1 && dz <= 65535 && h >= 1 && w >= 1 && nframes >= 0);
  SGNN_CHECK_ARG((int64_t)h * w <= ((int64_t)1 << 29));    // one frame's byte range fits a buffer resource
  if (nframes == 0) return SGNN_OK;
  SGNN_CHECK_ARG(sdf && weight && free_ctr && depth && frames && voxel_size > 0.f);
  FuseObb o{};
  if (obb) {
    o.on = 1;
    for (int c = 0; c < 3; ++c) o.a[c] = obb[c];
    for (int k = 0; k < 3; ++k) {
      for (int c = 0; c < 3; ++c) o.e[k][c] = obb[3 + 3 * k + c];
      o.ee[k] = (o.e[k][0] * o.e[k][0] + o.e[k][1] * o.e[k][1]) + o.e[k][2] * o.e[k][2];
    }
  }
  if (chunk <= 0 || chunk > nframes) chunk = nframes;
  const dim3 grid((dx + BRICK_X - 1) / BRICK_X, (dy + BRICK_Y - 1) / BRICK_Y, dz);
  for (int f0 = 0; f0 < nframes; f0 += chunk) {
    const int f1 = f0 + chunk < nframes ? f0 + chunk : nframes;
    SGNN_LAUNCH(k_fuse_integrate, grid, dim3(256), 0, (hipStream_t)stream, sdf, weight, free_ctr, dx, dy, depth, h, w,
                frames, f0, f1, voxel_size, depth_min, depth_max, o);
    SGNN_CHECK_LAUNCH();
  }
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_fuse_flag(const float *sdf, int dx, int dy, int dz, float keep_abs, float truncation,
                               float voxel_size, int64_t max_z, uint8_t *mask, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && dz >= 1 && max_z >= 0 && (truncation <= 0.f || voxel_size > 0.f));
  SGNN_CHECK_ARG(sdf && mask);
  const int64_t n = (int64_t)dx * dy * dz;
  SGNN_LAUNCH(k_fuse_flag, dim3(sgnn_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, sdf, n,
              (int64_t)dx * dy, keep_abs, truncation, voxel_size, max_z, mask);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_fuse_emit_block(const float *sdf, int dx, int dy, const int32_t *sel, const int64_t *count,
                                     int64_t n_max, uint32_t *locs_xyz, float *vals, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && n_max >= 0);
  if (n_max == 0) return SGNN_OK;
  SGNN_CHECK_ARG(sdf && sel && count && locs_xyz && vals);
  SGNN_LAUNCH(k_fuse_emit_block, dim3(sgnn_grid_for(n_max, 256, 8192)), dim3(256), 0, (hipStream_t)stream, sdf, dx, dy,
              sel, count, locs_xyz, vals);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_fuse_emit_rows(const float *sdf, int dx, int dy, float voxel_size, const int32_t *sel,
                                    const int64_t *count, int64_t n_max, int64_t *locs, float *feats,
                                    sgnn_stream_t stream) {
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && n_max >= 0 && voxel_size > 0.f);
  if (n_max == 0) return SGNN_OK;
  SGNN_CHECK_ARG(sdf && sel && count && locs && feats);
  SGNN_LAUNCH(k_fuse_emit_rows, dim3(sgnn_grid_for(n_max, 256, 8192)), dim3(256), 0, (hipStream_t)stream, sdf, dx, dy,
              voxel_size, sel, count, locs, feats);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_fuse_known(const float *sdf, int64_t n, float voxel_size, uint8_t *known, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && voxel_size > 0.f);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(sdf && known);
  SGNN_LAUNCH(k_fuse_known, dim3(sgnn_grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, sdf, n, voxel_size,
              known);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
