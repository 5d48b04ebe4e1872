// A depth sensor simulated on rendered frames (sgnn_amd.sensor): clean metric z-depth in, what a structured-light
// sensor with a horizontal baseline would have returned out.  The rules are listed in INTEGRATION.md section V; that
// text is the contract, and tests/sensor_ref.py restates it independently in NumPy.
//
// Kernels:
//   k_sensor_shadow   block = 4 waves = 4 image rows; a wave walks its row in 64-pixel chunks from the far end of the
//                     scan (rule V.5).  Inside a chunk the running minimum of the projector columns is a wave-level
//                     scan of six shuffle steps; between chunks it is one register.  No atomics, no LDS.  A negative
//                     baseline is the same scan over the mirrored row with negated columns, so there is one kernel.
//   k_sensor_degrade  one lane per output pixel, a wave per 8x8 pixel tile (block = 16x16 pixels of one frame), so
//                     that the jittered read and its four neighbours fall into the lines the tile holds anyway.  Reads
//                     the clean frame and the shadow mask, writes its own pixel and nothing else (rules V.1-V.9).
// Two launches: the shadow of a pixel depends on its whole row, the rest on a 5x5 window, and fusing the two would put
// a row scan in front of every tile.
//
// Every random quantity is an integer sum of hash bits scaled by one fp32 constant, every operation is a single fp32
// + - * / or a comparison: nothing here depends on the launch shape or on how frames are split over calls.
//
// Built with -ffp-contract=off (Makefile): every product and sum is rounded on its own.
#include <math.h>
#include "common.h"
#include "geom.h"   // finite_f and the pinhole of rule V.6

namespace {

constexpr int ROWS = 4;                        // rows (waves) per block of k_sensor_shadow
constexpr float C8 = 1.86881243e-05f;          // 1 / sqrt(8 (65536^2 - 1) / 12): eight 16-bit fields (rule V.2)
constexpr float C4 = 0.00676587503f;           // 1 / sqrt(4 (256^2 - 1) / 12): four 8-bit fields

// round half away from zero, exact: the integer part, stepped by one when the fraction (exact in fp32) reaches 1/2
__device__ __forceinline__ float round_away(float v) {
  const float t = truncf(v), r = v - t;
  if (r >= 0.5f) return t + 1.f;
  if (r <= -0.5f) return t - 1.f;
  return t;
}

// rule V.5.  key(p) of position p along the scan: p = x and key = u for baseline > 0, p = w - 1 - x and key = -u for
// baseline < 0; a pixel is in shadow iff a valid pixel at a later position has key <= its own.
__global__ __launch_bounds__(ROWS * 64) void k_sensor_shadow(const float *__restrict__ depth,
                                                            const float *__restrict__ intr, int rows, int h, int w,
                                                            float baseline, uint8_t *__restrict__ mask) {
  const int lane = threadIdx.x & 63;
  const int row = (int)blockIdx.x * ROWS + (int)(threadIdx.x >> 6);
  if (row >= rows) return;                                       // whole wave
  const float fb = intr[4 * (row / h)] * baseline;
  const bool flip = baseline < 0.f, on = baseline != 0.f;
  const float *d = depth + (int64_t)row * w;
  uint8_t *m = mask + (int64_t)row * w;
  float carry = INFINITY;                                        // min of the keys of every later chunk
  for (int c = (w - 1) >> 6; c >= 0; --c) {
    const int p = c * 64 + lane, x = flip ? w - 1 - p : p;
    const bool in = p < w;
    const float z = in ? d[x] : -INFINITY;
    const bool valid = on && finite_f(z) && z > 0.f;
    const float u = (float)x - __fdiv_rn(fb, z);
    const float key = valid ? (flip ? -u : u) : INFINITY;
    float run = key;                                             // -> min of the keys of lanes >= this one
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const float t = __shfl_down(run, s);
      if (lane + s < 64) run = fminf(run, t);
    }
    float later = __shfl_down(run, 1);                           // lanes > this one
    if (lane == 63) later = INFINITY;
    later = fminf(later, carry);
    if (in) m[x] = valid && later <= key;
    carry = fminf(carry, __shfl(run, 0));
  }
}

// rule V.2: the sum of the eight 16-bit fields of two draws, centred and scaled
__device__ __forceinline__ float gauss8(uint64_t a, uint64_t b) {
  int s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) s += (int)((a >> (16 * k)) & 0xffffu) + (int)((b >> (16 * k)) & 0xffffu);
  return (float)(s - 262140) * C8;
}

// the sum of the four 8-bit fields of 32 bits, centred and scaled
__device__ __forceinline__ float gauss4(uint32_t a) {
  const int s = (int)(a & 0xffu) + (int)((a >> 8) & 0xffu) + (int)((a >> 16) & 0xffu) + (int)(a >> 24);
  return (float)(s - 510) * C4;
}

// rule V.3 for one axis
__device__ __forceinline__ int jitter(float sigma, uint32_t bits) {
  const float j = round_away(sigma * gauss4(bits));
  return (int)fminf(fmaxf(j, -2.f), 2.f);
}

__global__ __launch_bounds__(256) void k_sensor_degrade(const float *__restrict__ depth,
                                                       const uint8_t *__restrict__ mask,
                                                       const float *__restrict__ intr,
                                                       const int64_t *__restrict__ frame_ids, int h, int w, int tx,
                                                       int ty, sgnn_sensor_model M, uint64_t base,
                                                       float *__restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned b = blockIdx.x;
  const int bx = (int)(b % (unsigned)tx), by = (int)((b / (unsigned)tx) % (unsigned)ty);
  const int fi = (int)(b / (unsigned)tx / (unsigned)ty);
  const int x = bx * 16 + (wave & 1) * 8 + (lane & 7), y = by * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (x >= w || y >= h) return;
  const int64_t frame0 = (int64_t)fi * h * w;
  const uint64_t f = frame_ids ? (uint64_t)frame_ids[fi] : (uint64_t)fi;
  const uint64_t at = base + ((f * (uint64_t)h + (uint64_t)y) * (uint64_t)w + (uint64_t)x) * 4u;   // rule V.1
  float res = -INFINITY;
  do {
    // V.3
    int sx = x, sy = y;
    if (M.lateral_sigma != 0.f) {
      const uint64_t r2 = sgnn_hash64(at + 2u);
      sx += jitter(M.lateral_sigma, (uint32_t)r2);
      sy += jitter(M.lateral_sigma, (uint32_t)(r2 >> 32));
      if (sx < 0 || sx >= w || sy < 0 || sy >= h) break;
    }
    const float *p = depth + frame0 + (int64_t)sy * w + sx;
    // V.4
    const float z = p[0];
    if (!finite_f(z) || z < M.min_depth || z > M.max_depth) break;
    // V.5
    const bool stereo = M.baseline != 0.f;
    if (stereo && mask[frame0 + (int64_t)sy * w + sx]) break;
    const float K[4] = {intr[4 * fi + 0], intr[4 * fi + 1], intr[4 * fi + 2], intr[4 * fi + 3]};   // fx, fy, cx, cy
    const bool noise = M.a0 != 0.f || M.a1 != 0.f;
    const uint64_t r3 = sgnn_hash64(at + 3u);
    // V.6
    float t = 0.f;
    if (noise || M.cos_min > 0.f || M.edge_drop > 0.f) {
      bool edge = !(sx >= 1 && sx + 1 < w && sy >= 1 && sy + 1 < h);
      float c2 = 0.f;
      if (!edge) {
        const float dl = p[-1], dr = p[1], du = p[-w], dd = p[w];
        edge = !(finite_f(dl) && finite_f(dr) && finite_f(du) && finite_f(dd));
        if (!edge) {
          const float xl = geom_unproject(K, 0, (float)(sx - 1)), xc = geom_unproject(K, 0, (float)sx);
          const float xr = geom_unproject(K, 0, (float)(sx + 1));
          const float yu = geom_unproject(K, 1, (float)(sy - 1)), yc = geom_unproject(K, 1, (float)sy);
          const float yd = geom_unproject(K, 1, (float)(sy + 1));
          // a = p(x+1, y) - p(x-1, y), b = p(x, y+1) - p(x, y-1), n = a x b, v = p(x, y)
          const float ax = xr * dr - xl * dl, ay = yc * dr - yc * dl, az = dr - dl;
          const float bx_ = xc * dd - xc * du, by_ = yd * dd - yu * du, bz = dd - du;
          const float nx = ay * bz - az * by_, ny = az * bx_ - ax * bz, nz = ax * by_ - ay * bx_;
          const float vx = xc * z, vy = yc * z;
          const float nn = (nx * nx + ny * ny) + nz * nz, vv = (vx * vx + vy * vy) + z * z;
          const float nv = (nx * vx + ny * vy) + nz * z;
          const float den = nn * vv;
          edge = !(den > 0.f && den < INFINITY);
          if (!edge) c2 = __fdiv_rn(nv * nv, den);
        }
      }
      if (edge) {
        if ((uint64_t)(uint32_t)r3 < (uint64_t)(M.edge_drop * 4294967296.f)) break;
      } else {
        if (c2 < M.cos_min * M.cos_min) break;
        const float tan2 = __fdiv_rn(1.f - c2, c2);
        t = tan2 > 0.f ? tan2 : 0.f;
      }
    }
    // V.7
    if ((r3 >> 32) < (uint64_t)(M.drop * 4294967296.f)) break;
    // V.8
    float z1 = z;
    if (noise) {
      const float g = gauss8(sgnn_hash64(at), sgnn_hash64(at + 1u));
      const float dz = z - M.a2;
      const float sigma = (M.a0 + (M.a1 * dz) * dz) * (1.f + M.a3 * t);
      z1 = z + sigma * g;
      if (!(z1 > 0.f && z1 < INFINITY)) break;
    }
    // V.9
    float z2 = z1;
    if (stereo && M.disparity_quantum != 0.f) {
      const float B = K[0] * fabsf(M.baseline);
      const float dq = round_away(__fdiv_rn(__fdiv_rn(B, z1), M.disparity_quantum)) * M.disparity_quantum;
      z2 = __fdiv_rn(B, dq);
      if (!(dq > 0.f && z2 > 0.f && z2 < INFINITY)) break;
    }
    res = z2;
  } while (false);
  out[frame0 + (int64_t)y * w + x] = res;
}

bool frames_ok(int nframes, int h, int w) {
  return nframes >= 0 && h >= 0 && w >= 0 && (int64_t)nframes * h < ((int64_t)1 << 31) &&
         (int64_t)nframes * h * w < ((int64_t)1 << 31);
}

bool unit_range(float v) { return v >= 0.f && v <= 1.f; }

}  // namespace

SGNN_EXPORT int sgnn_sensor_shadow(const float *depth, int nframes, int h, int w, const float *intrinsics,
                                   float baseline, uint8_t *mask, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(frames_ok(nframes, h, w));
  SGNN_CHECK_ARG(fabsf(baseline) < INFINITY);
  if ((int64_t)nframes * h * w == 0) return SGNN_OK;
  SGNN_CHECK_ARG(depth && intrinsics && mask);
  const int rows = nframes * h;
  SGNN_LAUNCH(k_sensor_shadow, dim3((unsigned)((rows + ROWS - 1) / ROWS)), dim3(ROWS * 64), 0, (hipStream_t)stream,
              depth, intrinsics, rows, h, w, baseline, mask);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_sensor_degrade(const float *depth, const uint8_t *mask, int nframes, int h, int w,
                                    const float *intrinsics, const int64_t *frame_ids, const sgnn_sensor_model *m,
                                    uint64_t seed, float *out, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(frames_ok(nframes, h, w));
  SGNN_CHECK_ARG(m != nullptr);
  SGNN_CHECK_ARG(m->lateral_sigma >= 0.f && m->lateral_sigma < INFINITY);
  SGNN_CHECK_ARG(m->min_depth <= m->max_depth);                  // either may be infinite; a NaN fails
  SGNN_CHECK_ARG(fabsf(m->baseline) < INFINITY);
  SGNN_CHECK_ARG(unit_range(m->cos_min) && unit_range(m->edge_drop) && unit_range(m->drop));
  SGNN_CHECK_ARG(fabsf(m->a0) < INFINITY && fabsf(m->a1) < INFINITY && fabsf(m->a2) < INFINITY &&
                 fabsf(m->a3) < INFINITY);
  SGNN_CHECK_ARG(m->disparity_quantum >= 0.f && m->disparity_quantum < INFINITY);
  if ((int64_t)nframes * h * w == 0) return SGNN_OK;
  SGNN_CHECK_ARG(depth && intrinsics && out && depth != out);
  SGNN_CHECK_ARG(mask || m->baseline == 0.f);
  const int tx = (w + 15) / 16, ty = (h + 15) / 16;
  const int64_t blocks = (int64_t)tx * ty * nframes;
  SGNN_CHECK_ARG(blocks < ((int64_t)1 << 31));
  // the hash of the seed on the host: the murmur3 finaliser of common.h
  uint64_t k = seed;
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  SGNN_LAUNCH(k_sensor_degrade, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, depth, mask, intrinsics,
              frame_ids, h, w, tx, ty, *m, k, out);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
