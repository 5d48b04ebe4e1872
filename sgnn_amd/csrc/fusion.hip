// TSDF fusion of depth frames into a scan volume (SG-NN's data generation: datagen/GenerateScans, the step before the
// .sdf / .knw files that io.hip reads).  The rules restated here are listed in INTEGRATION.md "TSDF fusion"; the
// reference's Fuser / VoxelGrid / CameraUtil depend on a library that is not part of this project, so those rules are
// the contract, and tests/fusion_ref.py restates them independently in NumPy.
//
// Kernels:
//   k_fuse_depth_raw      uint16 frames -> metric fp32 depth (nearest-index resampling, range test)     1 thread / pixel
//   k_fusecol_pack        uint8 RGB / RGBA frames -> RGBA frames on the depth frames' pixel grid        1 thread / pixel
//   k_fuse_bilateral      edge-preserving filter of the metric frames                                   1 thread / pixel
//   k_fuse_integrate      the hot path: every voxel folds a chunk of frames in input order, its (sdf, weight, free
//                         counter) in registers; state is read and written once per chunk.  <COLOR = true> also
//                         folds the frames' colour into an 8-byte (R, G, B, weight) record per voxel
//   k_fusecol_export      colour records -> uint8 RGB (the colour volume marching cubes takes) and colour weights
//   k_fuse_flag           |sdf| <= keep (the sparse file filter), optionally |sdf/vs| < truncation and z < max_z
//   k_fuse_emit_block     kept voxels -> (x,y,z) u32 + metric sdf f32, the .sdf block layout
//   k_fuse_emit_rows      kept voxels -> [z,y,x,0] int64 rows + sdf/vs features (the collated scene input)
//   k_fuse_known          u8 known codes of the .knw file
// Compaction between flag and emit is sgnn_compact_mask (stable: raster order, x fastest).  What this file shares with
// points.hip and regrid.hip is written once in tsdf.h: the OBB test, the observation rule (truncation, clamp, weight
// ramp) and the colour record's layout; the affine row and the projection: geom.h.  The per-frame float fold is its own.
//
// Built with -ffp-contract=off (Makefile): every product and sum below is rounded on its own, so the fp32
// restatement in the tests reproduces sdf, weight, free counter and colour record bit for bit.
#include <math.h>
#include "common.h"
#include "tsdf.h"

namespace {

// workgroup brick of the integration: 64 x 4 x 1 voxels, x contiguous (state loads / stores coalesce)
constexpr int BRICK_X = 64, BRICK_Y = 4;

__device__ __forceinline__ bool box_hits_brick(const int32_t *b, int x0, int x1, int y0, int y1, int k) {
  return b[0] <= x1 && b[1] >= x0 && b[2] <= y1 && b[3] >= y0 && b[4] <= k && b[5] >= k;
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

// the resampling of k_fuse_depth_raw for colour frames of `ch` = 3 or 4 bytes per pixel: out = R | G << 8 | B << 16 |
// A << 24 (memory order R, G, B, A), A = 255 for 3 channels and (a != 0) ? 255 : 0 for 4
__global__ __launch_bounds__(256) void k_fusecol_pack(const uint8_t *__restrict__ raw, int64_t npix, int hr, int wr,
                                                     int ch, int h, int w, uint32_t *__restrict__ out) {
  const float fx = __fdiv_rn((float)(wr - 1), (float)(w - 1));
  const float fy = __fdiv_rn((float)(hr - 1), (float)(h - 1));
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += stride) {
    const int64_t f = p / ((int64_t)h * w);
    const int r = (int)(p - f * h * w);
    const int j = r / w, i = r - j * w;
    int x = (int)roundf((float)i * fx), y = (int)roundf((float)j * fy);
    x = min(x, wr - 1);
    y = min(y, hr - 1);
    const uint8_t *s = raw + ((f * hr + y) * wr + x) * ch;
    const uint32_t a = (ch == 3 || s[3] != 0) ? 255u : 0u;
    out[p] = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | a << 24;
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
//
// COLOR: `color` holds one record per voxel (tsdf.h); `rgba` is the colour stack, 4 bytes per pixel on the depth stack's
// pixel grid, so a pixel has the same byte offset in both.  A sample that was not clamped on the free-space side and
// whose pixel has A != 0 folds its colour with the weight of the geometry update.  The colour fetch sits behind all the
// tests: only lanes that will use it ask for it.
template <bool COLOR>
__global__ __launch_bounds__(256) void k_fuse_integrate(float *__restrict__ sdf, uint8_t *__restrict__ weight,
                                                       int32_t *__restrict__ freec, uint2 *__restrict__ color,
                                                       int dx, int dy, const float *__restrict__ depth,
                                                       const uint8_t *__restrict__ rgba, int h, int w,
                                                       const sgnn_fuse_frame *__restrict__ fr, int f0, int f1,
                                                       float vs, float dmin, float dmax, TsdfObb obb) {
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
  float q[3] = {0.f, 0.f, 0.f};                                            // integer-valued: what is stored and reloaded
  int wc = 0;
  if (inside) {
    s = sdf[v];
    wt = weight[v];
    fc = freec[v];
    if constexpr (COLOR) {
      const TsdfColor c = tsdf_color_unpack(color[v]);
#pragma unroll
      for (int t = 0; t < 3; ++t) q[t] = (float)c.q[t];
      wc = (int)c.w;
    }
  }
  const float fi = (float)i, fj = (float)j, fk = (float)k;
  const bool eligible = inside && (!obb.on || tsdf_obb_contains(obb, fi, fj, fk));
  const uint32_t frame_bytes = (uint32_t)h * (uint32_t)w * 4u;

  for (int f = f0; f < f1; ++f) {
    const sgnn_fuse_frame &F = fr[f];
    if (!box_hits_brick(F.box, x0, x1, y0, y1, k)) continue;
    const bool inbox = eligible && i >= F.box[0] && i <= F.box[1] && j >= F.box[2] && j <= F.box[3];
    const float px3 = tsdf_affine_row(F.m, 0, fi, fj, fk), py3 = tsdf_affine_row(F.m, 1, fi, fj, fk);
    const float pz = tsdf_affine_row(F.m, 2, fi, fj, fk);
    const float px = geom_project(F.intr, 0, px3, pz), py = geom_project(F.intr, 1, py3, pz);
    const float rx = roundf(px), ry = roundf(py);                        // NaN / inf fail both range tests
    const bool on_image = inbox && rx >= 0.f && rx < (float)w && ry >= 0.f && ry < (float)h;
    // pixels off the image read at an out-of-range offset: the buffer load returns 0, which fails the range test
    const uint32_t off = on_image ? ((uint32_t)ry * (uint32_t)w + (uint32_t)rx) * 4u : 0xFFFFFFFFu;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(depth + F.offset), 0, (int)frame_bytes, 0x00020000);
    const float d = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
    if (!(on_image && d >= dmin && d <= dmax)) continue;
    if (pz < d) ++fc;                                                     // voxel in front of the observation
    const float sd0 = d - pz;
    const float trunc = tsdf_trunc(vs, d);
    if (!(sd0 > -trunc)) continue;
    const float sd = tsdf_clamp_sd(sd0, trunc), wu = tsdf_ramp(d);
    if (s == -INFINITY) s = sd;
    else s = __fdiv_rn(s * (float)wt + sd * wu, (float)wt + wu);
    wt = min(wt + (int)wu, 255);
    if constexpr (COLOR) {
      if (!(sd0 < trunc)) continue;                                       // free space gets no colour
      const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<uint8_t *>(rgba + F.offset * 4), 0, (int)frame_bytes, 0x00020000);
      const uint32_t px4 = __builtin_amdgcn_raw_buffer_load_b32(rc, off, 0, 0);
      if ((px4 >> 24) == 0u) continue;                                    // A == 0: the pixel has no colour
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float ci = (float)(((px4 >> (8 * c)) & 0xFFu) * 256u);
        if (wc == 0) q[c] = ci;
        else q[c] = roundf(__fdiv_rn(q[c] * (float)wc + ci * wu, (float)wc + wu));
      }
      wc = min(wc + (int)wu, 255);
    }
  }
  if (inside) {
    sdf[v] = s;
    weight[v] = (uint8_t)wt;
    freec[v] = fc;
    if constexpr (COLOR) {
      color[v] = tsdf_color_pack((uint32_t)q[0], (uint32_t)q[1], (uint32_t)q[2], (uint32_t)wc);
    }
  }
}

// c8 = (q + 128) >> 8 where the colour weight is positive, else 0.  One thread takes four voxels: 32 bytes in, 12 + 4 out.
__global__ __launch_bounds__(256) void k_fusecol_export(const uint2 *__restrict__ color, int64_t n,
                                                       uint8_t *__restrict__ rgb, uint8_t *__restrict__ wcout) {
  const int64_t groups = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += stride) {
    const int64_t v0 = 4 * g;
    const int m = (int)(n - v0 < 4 ? n - v0 : 4);
    uint8_t o[12];
    uint8_t wq[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const TsdfColor c = tsdf_color_unpack(t < m ? color[v0 + t] : make_uint2(0u, 0u));
      wq[t] = (uint8_t)c.w;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o[3 * t + ch] = c.w ? (uint8_t)tsdf_color8(c.q[ch]) : 0;
    }
    if (m == 4) {                                                         // rgb + 12 g and wcout + 4 g are 4-byte aligned
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        reinterpret_cast<uint32_t *>(rgb + 3 * v0)[t] = (uint32_t)o[4 * t] | (uint32_t)o[4 * t + 1] << 8 |
                                                        (uint32_t)o[4 * t + 2] << 16 | (uint32_t)o[4 * t + 3] << 24;
      }
      if (wcout) {
        *reinterpret_cast<uint32_t *>(wcout + v0) =
            (uint32_t)wq[0] | (uint32_t)wq[1] << 8 | (uint32_t)wq[2] << 16 | (uint32_t)wq[3] << 24;
      }
    } else {
      for (int t = 0; t < 3 * m; ++t) rgb[3 * v0 + t] = o[t];
      for (int t = 0; t < m && wcout; ++t) wcout[v0 + t] = wq[t];
    }
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

SGNN_EXPORT int sgnn_fusecol_pack(const uint8_t *raw, int nframes, int h_raw, int w_raw, int channels, int h, int w,
                                  uint8_t *out, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nframes >= 0 && h_raw >= 2 && w_raw >= 2 && h >= 2 && w >= 2 && (channels == 3 || channels == 4));
  if (nframes == 0) return SGNN_OK;
  SGNN_CHECK_ARG(raw && out && raw != out && ((uintptr_t)out & 3) == 0);
  const int64_t npix = (int64_t)nframes * h * w;
  SGNN_LAUNCH(k_fusecol_pack, dim3(sgnn_grid_for(npix, 256, 8192)), dim3(256), 0, (hipStream_t)stream, raw, npix, h_raw,
              w_raw, channels, h, w, reinterpret_cast<uint32_t *>(out));
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

// the one host side of both integrate entry points; color / rgba NULL = the depth-only instantiation
static int fuse_integrate(float *sdf, uint8_t *weight, int32_t *free_ctr, uint16_t *color, int dx, int dy, int dz,
                          const float *depth, const uint8_t *rgba, int h, int w, const sgnn_fuse_frame *frames,
                          int nframes, int chunk, float voxel_size, float depth_min, float depth_max, const float *obb,
                          sgnn_stream_t stream) {
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && dz >= 1 && dz <= 65535 && h >= 1 && w >= 1 && nframes >= 0);
  SGNN_CHECK_ARG((int64_t)h * w <= ((int64_t)1 << 29));    // one frame's byte range fits a buffer resource
  if (nframes == 0) return SGNN_OK;
  TsdfVol vol;
  SGNN_CHECK_ARG(tsdf_vol_arg(sdf, weight, free_ctr, color, vol) && depth && frames && voxel_size > 0.f);
  SGNN_CHECK_ARG((color != nullptr) == (rgba != nullptr) && ((uintptr_t)rgba & 3) == 0);
  const TsdfObb o = tsdf_obb_arg(obb);
  if (chunk <= 0 || chunk > nframes) chunk = nframes;
  const dim3 grid((dx + BRICK_X - 1) / BRICK_X, (dy + BRICK_Y - 1) / BRICK_Y, dz);
  const auto kernel = color ? k_fuse_integrate<true> : k_fuse_integrate<false>;
  for (int f0 = 0; f0 < nframes; f0 += chunk) {
    const int f1 = f0 + chunk < nframes ? f0 + chunk : nframes;
    SGNN_LAUNCH(kernel, grid, dim3(256), 0, (hipStream_t)stream, vol.sdf, vol.weight, vol.freec, vol.color, dx, dy, depth,
                rgba, h, w, frames, f0, f1, voxel_size, depth_min, depth_max, o);
    SGNN_CHECK_LAUNCH();
  }
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_fuse_integrate(float *sdf, uint8_t *weight, int32_t *free_ctr, int dx, int dy, int dz,
                                    const float *depth, int h, int w, const sgnn_fuse_frame *frames, int nframes,
                                    int chunk, float voxel_size, float depth_min, float depth_max, const float *obb,
                                    sgnn_stream_t stream) {
  return fuse_integrate(sdf, weight, free_ctr, nullptr, dx, dy, dz, depth, nullptr, h, w, frames, nframes, chunk,
                        voxel_size, depth_min, depth_max, obb, stream);
}

SGNN_EXPORT int sgnn_fusecol_integrate(float *sdf, uint8_t *weight, int32_t *free_ctr, uint16_t *color, int dx, int dy,
                                       int dz, const float *depth, const uint8_t *rgba, int h, int w,
                                       const sgnn_fuse_frame *frames, int nframes, int chunk, float voxel_size,
                                       float depth_min, float depth_max, const float *obb, sgnn_stream_t stream) {
  if (nframes > 0) SGNN_CHECK_ARG(color && rgba);
  return fuse_integrate(sdf, weight, free_ctr, color, dx, dy, dz, depth, rgba, h, w, frames, nframes, chunk,
                        voxel_size, depth_min, depth_max, obb, stream);
}

SGNN_EXPORT int sgnn_fusecol_export(const uint16_t *color, int64_t n, uint8_t *rgb, uint8_t *wc, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(color && rgb && ((uintptr_t)color & 7) == 0 && ((uintptr_t)rgb & 3) == 0 && ((uintptr_t)wc & 3) == 0);
  SGNN_LAUNCH(k_fusecol_export, dim3(sgnn_grid_for((n + 3) / 4, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
              reinterpret_cast<const uint2 *>(color), n, rgb, wc);
  SGNN_CHECK_LAUNCH();
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
