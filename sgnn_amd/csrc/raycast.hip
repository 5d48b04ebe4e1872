// TSDF volumes ray-cast to depth and normal frames (sgnn_amd.raycast): the "model to frame" half that goes with the
// fuser of fusion.hip.  The rules are listed in INTEGRATION.md section H; that text is the contract, and
// tests/raycast_ref.py restates it independently in NumPy.
//
// Kernels:
//   k_raycast_bricks  one byte per 8x8x8 brick: does it hold a usable voxel (|sdf| < band)?  A wave covers 8 bricks
//                     along x, a (z, y) row of 64 voxels per iteration, one ballot per row (the shape of
//                     k_chunk_score).
//   k_raycast         grid = (16x16 pixel blocks, frames of the launch).  A lane owns one ray, a wave an 8x8 pixel
//                     tile of one frame, so the eight corner loads of a wave fall into few cache lines; the frame
//                     record is wave-uniform and arrives by scalar loads.  Lanes of a tile finish at different
//                     samples; a wave leaves its loop when its last lane is done.
//
// Skipping (rule 7).  A sample whose cell lies outside the volume, or in a brick without a usable voxel, is invalid by
// rule 4 whatever its eight corners hold.  From such a sample k the ray estimates the sample kn at which it leaves
// that region (the slab exit, minus a safety sample) and then CHECKS sample kn - 1: every coordinate of a sample is
// a monotonic function of k (t_k = depth_min + (float)k * dt and g = o + t * d are single rounded operations, each
// monotonic in its argument), so if samples k and kn - 1 both lie in the region, which is a box in grid space,
// every sample between them does.  A failed check skips sample k alone.  Nothing rests on the accuracy of the
// estimate: the result is the one of the plain walk, bit for bit.
//
// Colour frames of a volume that carries a colour per voxel come from the same kernel text (template parameter
// COLOR, rules in INTEGRATION.md section N, restated in tests/raycast_color_ref.py): a lane that has a hit fetches
// the eight R, G, B, A words of the hit's cell once, after the walk.
//
// The differentiable cast (restated in tests/raycast_grad_ref.py) is the same kernel text
// once more (template parameter DIFF): depth is k_raycast's, and a lane also keeps the sample index of its hit,
// reads a per-voxel feature vector at the hit and says whether the hit's cell is whole.
//   k_raycast_grad    the backward: the forward's geometry, one lane per pixel and a wave per 8x8 tile, so a wave's
//                     atomics fall into few rows of the gradient volumes.  A lane rebuilds both samples of its
//                     crossing from the recorded index (a sample's position is a product, never a running sum) and
//                     scatters sixteen terms into grad_sdf and eight per channel into grad_features with
//                     no-return fp32 atomic adds.
//
// Built with -ffp-contract=off (Makefile): every product and sum is rounded on its own.
#include <math.h>
#include "common.h"

namespace {

constexpr int BRICK = 8;   // edge of a brick of the skip table

struct Volume {
  const float *sdf;
  int dx, dy, dz;
  float band;
};

// rule 4: the sample at grid position g; false = invalid
__device__ __forceinline__ bool sample(const Volume &V, float gx, float gy, float gz, float &v) {
  const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
  v = 0.f;
  if (!(fx >= 0.f && fx <= (float)(V.dx - 2) && fy >= 0.f && fy <= (float)(V.dy - 2) && fz >= 0.f &&
        fz <= (float)(V.dz - 2)))
    return false;                                   // NaN fails
  const int64_t sy = V.dx, sz = (int64_t)V.dx * V.dy;
  const float *p = V.sdf + ((int64_t)(int)fz * V.dy + (int)fy) * V.dx + (int)fx;
  const float c000 = p[0], c001 = p[1], c010 = p[sy], c011 = p[sy + 1];
  const float c100 = p[sz], c101 = p[sz + 1], c110 = p[sz + sy], c111 = p[sz + sy + 1];
  const float b = V.band;                           // |c| < band is false for a NaN and for an infinity
  if (!(fabsf(c000) < b && fabsf(c001) < b && fabsf(c010) < b && fabsf(c011) < b && fabsf(c100) < b &&
        fabsf(c101) < b && fabsf(c110) < b && fabsf(c111) < b))
    return false;
  const float ax = gx - fx, ay = gy - fy, az = gz - fz;
  const float x00 = c000 + ax * (c001 - c000), x01 = c010 + ax * (c011 - c010);
  const float x10 = c100 + ax * (c101 - c100), x11 = c110 + ax * (c111 - c110);
  const float y0 = x00 + ay * (x01 - x00), y1 = x10 + ay * (x11 - x10);
  v = y0 + az * (y1 - y0);
  return true;
}

// Section N: the colour at the hit g, from the cell's corners that have one (A != 0); the R, G, B, A bytes of the
// pixel as one word, 0 = no colour.  colors is the dense (dz, dy, dx) volume of R, G, B, A words.
__device__ __forceinline__ uint32_t hit_color(const Volume &V, const uint32_t *__restrict__ colors, float gx, float gy,
                                              float gz) {
  const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
  if (!(fx >= 0.f && fx <= (float)(V.dx - 2) && fy >= 0.f && fy <= (float)(V.dy - 2) && fz >= 0.f &&
        fz <= (float)(V.dz - 2)))
    return 0u;
  const int64_t sy = V.dx, sz = (int64_t)V.dx * V.dy;
  const uint32_t *p = colors + ((int64_t)(int)fz * V.dy + (int)fy) * V.dx + (int)fx;
  uint32_t c[8];                                    // x fastest, then y, then z
#pragma unroll
  for (int i = 0; i < 8; ++i) c[i] = p[(i >> 2) * sz + ((i >> 1) & 1) * sy + (i & 1)];
  const float ax = gx - fx, ay = gy - fy, az = gz - fz;
  const float wx[2] = {1.0f - ax, ax}, wy[2] = {1.0f - ay, ay}, wz[2] = {1.0f - az, az};
  float s = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    // a corner without a colour adds a weight of zero: the sums are those over the counted corners, bit for bit
    const float w = (c[i] >> 24) ? (wz[i >> 2] * wy[(i >> 1) & 1]) * wx[i & 1] : 0.f;
    s = s + w;
    n0 = n0 + w * (float)(c[i] & 255u);
    n1 = n1 + w * (float)((c[i] >> 8) & 255u);
    n2 = n2 + w * (float)((c[i] >> 16) & 255u);
  }
  if (s == 0.f) return 0u;
  auto ch = [](float v) {
    const float r = roundf(v);                      // half away from zero
    return r >= 255.0f ? 255u : (r >= 0.0f ? (uint32_t)r : 0u);
  };
  return ch(__fdiv_rn(n0, s)) | (ch(__fdiv_rn(n1, s)) << 8) | (ch(__fdiv_rn(n2, s)) << 16) | 0xFF000000u;
}

// offset of corner i of a cell (x fastest, then y, then z) from its corner f, in voxels
__device__ __forceinline__ int64_t corner_offset(const Volume &V, int i) {
  return (int64_t)(i >> 2) * V.dx * V.dy + (int64_t)((i >> 1) & 1) * V.dx + (i & 1);
}

// Section U rule 3: the cell of g and its axis weights {1 - a, a}; false when the cell test fails (NaN fails)
struct Cell {
  int64_t base;       // voxel index of corner f
  float wx[2], wy[2], wz[2];
  __device__ __forceinline__ float weight(int i) const { return (wz[i >> 2] * wy[(i >> 1) & 1]) * wx[i & 1]; }
};

__device__ __forceinline__ bool cell_of(const Volume &V, float gx, float gy, float gz, Cell &c) {
  const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
  if (!(fx >= 0.f && fx <= (float)(V.dx - 2) && fy >= 0.f && fy <= (float)(V.dy - 2) && fz >= 0.f &&
        fz <= (float)(V.dz - 2)))
    return false;
  c.base = ((int64_t)(int)fz * V.dy + (int)fy) * V.dx + (int)fx;
  const float ax = gx - fx, ay = gy - fy, az = gz - fz;
  c.wx[0] = 1.0f - ax, c.wx[1] = ax;
  c.wy[0] = 1.0f - ay, c.wy[1] = ay;
  c.wz[0] = 1.0f - az, c.wz[1] = az;
  return true;
}

// what k_raycast<.., DIFF = true> reads and writes beside depth
struct Diff {
  const float *features;   // (dz, dy, dx, channels), or null
  int channels;
  int32_t *hit;            // (F, h, w): the sample index of the hit, -1 = none
  float *feat;             // (F, h, w, channels), or null
  uint8_t *ok;             // (F, h, w)
};

struct Ray {
  float ox, oy, oz;   // origin (grid)
  float dx, dy, dz;   // direction per unit of z-depth (grid)
  float t0, dt;       // sample k sits at t0 + (float)k * dt
};

// the first sample at or after depth tc, less one: where a jump that started before tc has to stop (k + 1 at least)
__device__ __forceinline__ int jump_target(const Ray &R, float tc, int k, int n) {
  const float q = floorf(__fdiv_rn(tc - R.t0, R.dt));
  if (!(q > (float)(k + 1))) return k + 1;          // NaN: one sample
  return q < (float)n ? (int)q : n;
}

// Rule 7 for sample k at g: k when the sample has to be evaluated, else the next sample to look at (> k); samples
// k .. result - 1 are invalid by rule 4.
__device__ __forceinline__ int skip_from(const Volume &V, const uint8_t *__restrict__ bricks, int nbx, int nby,
                                         const Ray &R, float gx, float gy, float gz, int k, int n) {
  const float lx = (float)(V.dx - 1), ly = (float)(V.dy - 1), lz = (float)(V.dz - 1);   // cell f is in range iff 0 <= g < l
  const bool in = gx >= 0.f && gx < lx && gy >= 0.f && gy < ly && gz >= 0.f && gz < lz;
  if (!in) {
    // outside on one axis at least: the half-space g_a < 0 or g_a >= l_a holds no valid sample
    float oa, da, bound;
    bool high;
    if (gx < 0.f || gx >= lx) { oa = R.ox; da = R.dx; high = gx >= lx; bound = high ? lx : 0.f; }
    else if (gy < 0.f || gy >= ly) { oa = R.oy; da = R.dy; high = gy >= ly; bound = high ? ly : 0.f; }
    else if (gz < 0.f || gz >= lz) { oa = R.oz; da = R.dz; high = gz >= lz; bound = high ? lz : 0.f; }
    else return k + 1;                              // a NaN coordinate
    const bool away = high ? da >= 0.f : da <= 0.f;   // never comes back: the rest of the ray
    const int kn = away ? n : jump_target(R, __fdiv_rn(bound - oa, da), k, n);
    if (kn == k + 1) return kn;
    const float ga = oa + (R.t0 + (float)(kn - 1) * R.dt) * da;
    return (high ? ga >= bound : ga < 0.f) ? kn : k + 1;
  }
  const int bx = (int)gx >> 3, by = (int)gy >> 3, bz = (int)gz >> 3;                    // g >= 0: truncation is floor
  if (bricks[((int64_t)bz * nby + by) * nbx + bx]) return k;
  // a dead brick: corner f of every cell in it is unusable
  const float x0 = (float)(bx * BRICK), y0 = (float)(by * BRICK), z0 = (float)(bz * BRICK);
  const float x1 = x0 + (float)BRICK, y1 = y0 + (float)BRICK, z1 = z0 + (float)BRICK;
  float tc = INFINITY;
  if (R.dx != 0.f) tc = fminf(tc, __fdiv_rn((R.dx > 0.f ? x1 : x0) - R.ox, R.dx));
  if (R.dy != 0.f) tc = fminf(tc, __fdiv_rn((R.dy > 0.f ? y1 : y0) - R.oy, R.dy));
  if (R.dz != 0.f) tc = fminf(tc, __fdiv_rn((R.dz > 0.f ? z1 : z0) - R.oz, R.dz));
  const int kn = jump_target(R, tc, k, n);
  if (kn == k + 1) return kn;
  const float t = R.t0 + (float)(kn - 1) * R.dt;
  const float hx = R.ox + t * R.dx, hy = R.oy + t * R.dy, hz = R.oz + t * R.dz;
  const bool same = hx >= x0 && hx < x1 && hy >= y0 && hy < y1 && hz >= z0 && hz < z1;
  return same ? kn : k + 1;
}

// block = 4 waves = 4 brick rows (y) of one brick slice (z); wave = 8 bricks along x; lane = x within those 64 voxels
__global__ __launch_bounds__(256) void k_raycast_bricks(const float *__restrict__ sdf, int dx, int dy, int dz, int nbx,
                                                       int nby, float band, uint8_t *__restrict__ bricks) {
  const int lane = threadIdx.x & 63;
  const int by = blockIdx.y * 4 + (int)(threadIdx.x >> 6), bz = blockIdx.z;
  if (by >= nby) return;                           // whole wave
  const int x = blockIdx.x * 64 + lane;
  const bool x_in = x < dx;
  unsigned long long any = 0;                      // byte b: lanes of brick blockIdx.x * 8 + b with a usable voxel
  for (int k = 0; k < BRICK; ++k) {
    const int z = bz * BRICK + k;
#pragma unroll
    for (int j = 0; j < BRICK; ++j) {
      const int y = by * BRICK + j;
      const bool in = x_in && y < dy && z < dz;
      const float s = sdf[in ? ((int64_t)z * dy + y) * dx + x : 0];
      any |= __ballot(in && fabsf(s) < band);
    }
  }
  const int bx = blockIdx.x * 8 + lane;
  if (lane < 8 && bx < nbx)
    bricks[((int64_t)bz * nby + by) * nbx + bx] = ((any >> (8 * lane)) & 0xFFull) ? 1 : 0;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;                                        // lane 0 holds the sum
}

template <bool SKIP, bool NORMALS, bool COLOR, bool DIFF>
__global__ __launch_bounds__(256) void k_raycast(Volume V, const uint8_t *__restrict__ bricks, int nbx, int nby,
                                                const sgnn_raycast_frame *__restrict__ frames, int f0, int h, int w,
                                                float depth_min, float dt, int nsamples, float *__restrict__ depth,
                                                float *__restrict__ normal,
                                                unsigned long long *__restrict__ counters,
                                                const uint32_t *__restrict__ colors, uint32_t *__restrict__ rgba,
                                                Diff D) {
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const int i = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int j = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  const int f = f0 + (int)blockIdx.z;
  const sgnn_raycast_frame &F = frames[f];
  const float *G = F.g;
  const bool pixel = i < w && j < h;
  const bool live = pixel && G[0] == G[0];          // non-finite pose (the host stores NaN): the frame stays empty
  // rule 2
  const float cx = __fdiv_rn((float)i - F.intr[2], F.intr[0]), cy = __fdiv_rn((float)j - F.intr[3], F.intr[1]);
  Ray R;
  R.dx = (G[0] * cx + G[1] * cy) + G[2];
  R.dy = (G[4] * cx + G[5] * cy) + G[6];
  R.dz = (G[8] * cx + G[9] * cy) + G[10];
  R.ox = G[3];
  R.oy = G[7];
  R.oz = G[11];
  R.t0 = depth_min;
  R.dt = dt;
  // rules 3-5
  const int n = live ? nsamples : 0;
  int k = 0, n_eval = 0, n_skip = 0;
  bool pvalid = false;
  float pv = 0.f, hit = -INFINITY;
  while (k < n) {
    const float t = R.t0 + (float)k * R.dt;
    const float gx = R.ox + t * R.dx, gy = R.oy + t * R.dy, gz = R.oz + t * R.dz;
    if (SKIP) {
      const int kn = skip_from(V, bricks, nbx, nby, R, gx, gy, gz, k, n);
      if (kn > k) {
        n_skip += kn - k;
        k = kn;
        pvalid = false;
        continue;
      }
    }
    float v;
    const bool valid = sample(V, gx, gy, gz, v);
    ++n_eval;
    if (valid && pvalid) {
      if (pv > 0.f && v <= 0.f) {
        hit = (R.t0 + (float)(k - 1) * R.dt) + R.dt * __fdiv_rn(pv, pv - v);
        break;
      }
      if (pv < 0.f && v > 0.f) break;               // the surface seen from behind
    }
    pvalid = valid;
    pv = v;
    ++k;
  }
  if (pixel) {
    const int64_t px = ((int64_t)f * h + j) * w + i;
    depth[px] = hit;
    if (NORMALS) {
      // rule 6
      float nx = NAN, ny = NAN, nz = NAN;
      if (hit > -INFINITY) {
        const float gx = R.ox + hit * R.dx, gy = R.oy + hit * R.dy, gz = R.oz + hit * R.dz;
        float xp, xm, yp, ym, zp, zm;
        bool ok = sample(V, gx + 0.5f, gy, gz, xp);
        ok = sample(V, gx - 0.5f, gy, gz, xm) && ok;
        ok = sample(V, gx, gy + 0.5f, gz, yp) && ok;
        ok = sample(V, gx, gy - 0.5f, gz, ym) && ok;
        ok = sample(V, gx, gy, gz + 0.5f, zp) && ok;
        ok = sample(V, gx, gy, gz - 0.5f, zm) && ok;
        if (ok) {
          const float a = xp - xm, b = yp - ym, c = zp - zm;
          const float qx = (G[0] * a + G[4] * b) + G[8] * c;
          const float qy = (G[1] * a + G[5] * b) + G[9] * c;
          const float qz = (G[2] * a + G[6] * b) + G[10] * c;
          const float len = (float)sqrt((double)((qx * qx + qy * qy) + qz * qz));   // correctly rounded
          if (len > 0.f && len < INFINITY) {
            nx = __fdiv_rn(qx, len);
            ny = __fdiv_rn(qy, len);
            nz = __fdiv_rn(qz, len);
          }
        }
      }
      normal[px * 3 + 0] = nx;
      normal[px * 3 + 1] = ny;
      normal[px * 3 + 2] = nz;
    }
    if (COLOR) {
      // section N: only a lane with a hit fetches colour, at the point of rule 6
      uint32_t c = 0u;
      if (hit > -INFINITY) c = hit_color(V, colors, R.ox + hit * R.dx, R.oy + hit * R.dy, R.oz + hit * R.dz);
      rgba[px] = c;
    }
    if (DIFF) {
      // section U rules 2 and 3: the hit's sample index; features and ok from the cell of the hit, read once
      const bool has = hit > -INFINITY;
      D.hit[px] = has ? k : -1;
      Cell c;
      const bool cell = has && cell_of(V, R.ox + hit * R.dx, R.oy + hit * R.dy, R.oz + hit * R.dz, c);
      bool ok = cell;
      if (cell) {
#pragma unroll
        for (int i = 0; i < 8; ++i) ok = (fabsf(V.sdf[c.base + corner_offset(V, i)]) < V.band) && ok;
      }
      D.ok[px] = ok ? 1 : 0;
      if (D.feat) {
        float wgt[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) wgt[i] = cell ? c.weight(i) : 0.f;
        for (int ch = 0; ch < D.channels; ++ch) {
          float acc = 0.f;
          if (cell) {
            const float *p = D.features + c.base * D.channels + ch;
            acc = wgt[0] * p[0];
#pragma unroll
            for (int i = 1; i < 8; ++i) acc = acc + wgt[i] * p[corner_offset(V, i) * D.channels];
          }
          D.feat[px * D.channels + ch] = acc;
        }
      }
    }
  }
  if (counters) {                                   // kernel argument: the same for every lane
    const long long e = wave_sum(n_eval), s = wave_sum(n_skip);
    if (lane == 0) {
      if (e) atomicAdd(counters + 0, (unsigned long long)e);
      if (s) atomicAdd(counters + 1, (unsigned long long)s);
    }
  }
}

// Section U rules 4 and 5: the backward of k_raycast<.., DIFF = true>.  hit is the forward's record; a pixel whose
// record is no sample index of the cast, or whose samples do not lie in cells of the volume (neither happens to a
// record the forward wrote), adds nothing, so that no record can make a lane write outside the gradient volumes.
__global__ __launch_bounds__(256) void k_raycast_grad(Volume V, const sgnn_raycast_frame *__restrict__ frames, int f0,
                                                     int h, int w, float depth_min, float dt, int nsamples,
                                                     const int32_t *__restrict__ hit,
                                                     const float *__restrict__ features, int channels,
                                                     const float *__restrict__ grad_depth,
                                                     const float *__restrict__ grad_feat, float *__restrict__ grad_sdf,
                                                     float *__restrict__ grad_features) {
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const int i = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int j = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  const int f = f0 + (int)blockIdx.z;
  if (!(i < w && j < h)) return;
  const sgnn_raycast_frame &F = frames[f];
  const float *G = F.g;
  const int64_t px = ((int64_t)f * h + j) * w + i;
  const int k = hit[px];
  if (!(G[0] == G[0]) || k < 1 || k >= nsamples) return;   // no hit: the incoming gradient is not even read
  // rule H2
  const float cx = __fdiv_rn((float)i - F.intr[2], F.intr[0]), cy = __fdiv_rn((float)j - F.intr[3], F.intr[1]);
  const float dx = (G[0] * cx + G[1] * cy) + G[2], dy = (G[4] * cx + G[5] * cy) + G[6];
  const float dz = (G[8] * cx + G[9] * cy) + G[10];
  const float ox = G[3], oy = G[7], oz = G[11];
  // rules H3 and H4: both samples of the crossing; every finite corner counts, the forward found them usable
  const float t0 = depth_min + (float)(k - 1) * dt, t1 = depth_min + (float)k * dt;
  const float g0x = ox + t0 * dx, g0y = oy + t0 * dy, g0z = oz + t0 * dz;
  const float g1x = ox + t1 * dx, g1y = oy + t1 * dy, g1z = oz + t1 * dz;
  float pv, v;
  Cell c0, c1;
  if (!(sample(V, g0x, g0y, g0z, pv) && sample(V, g1x, g1y, g1z, v))) return;   // V.band is infinite here
  cell_of(V, g0x, g0y, g0z, c0);
  cell_of(V, g1x, g1y, g1z, c1);
  const float den = pv - v;
  const float ts = t0 + dt * __fdiv_rn(pv, den);     // the forward's depth
  float Gs = grad_depth ? grad_depth[px] : 0.f;
  Cell cs;
  if (grad_feat && cell_of(V, ox + ts * dx, oy + ts * dy, oz + ts * dz, cs)) {
    float wgt[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) wgt[c] = cs.weight(c);
    for (int ch = 0; ch < channels; ++ch) {
      const float gf = grad_feat[px * channels + ch];
      const int64_t at = cs.base * channels + ch;
      float q[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) q[c] = features[at + corner_offset(V, c) * channels];
      // the gradient of rule 3's interpolant: four edges along each axis, in corner order
      float qx = (cs.wz[0] * cs.wy[0]) * (q[1] - q[0]);
      qx = qx + (cs.wz[0] * cs.wy[1]) * (q[3] - q[2]);
      qx = qx + (cs.wz[1] * cs.wy[0]) * (q[5] - q[4]);
      qx = qx + (cs.wz[1] * cs.wy[1]) * (q[7] - q[6]);
      float qy = (cs.wz[0] * cs.wx[0]) * (q[2] - q[0]);
      qy = qy + (cs.wz[0] * cs.wx[1]) * (q[3] - q[1]);
      qy = qy + (cs.wz[1] * cs.wx[0]) * (q[6] - q[4]);
      qy = qy + (cs.wz[1] * cs.wx[1]) * (q[7] - q[5]);
      float qz = (cs.wy[0] * cs.wx[0]) * (q[4] - q[0]);
      qz = qz + (cs.wy[0] * cs.wx[1]) * (q[5] - q[1]);
      qz = qz + (cs.wy[1] * cs.wx[0]) * (q[6] - q[2]);
      qz = qz + (cs.wy[1] * cs.wx[1]) * (q[7] - q[3]);
      Gs = Gs + gf * ((qx * dx + qy * dy) + qz * dz);
      if (grad_features) {
#pragma unroll
        for (int c = 0; c < 8; ++c) atomicAdd(grad_features + at + corner_offset(V, c) * channels, gf * wgt[c]);
      }
    }
  }
  if (!grad_sdf) return;
  const float A = __fdiv_rn(Gs * dt, den * den);
  const float cpv = A * (-v), cv = A * pv;
#pragma unroll
  for (int c = 0; c < 8; ++c) atomicAdd(grad_sdf + c0.base + corner_offset(V, c), cpv * c0.weight(c));
#pragma unroll
  for (int c = 0; c < 8; ++c) atomicAdd(grad_sdf + c1.base + corner_offset(V, c), cv * c1.weight(c));
}

}  // namespace

SGNN_EXPORT int sgnn_raycast_bricks(const float *sdf, int dx, int dy, int dz, float band, uint8_t *bricks,
                                    sgnn_stream_t stream) {
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && dz >= 1 && dx <= 65535 && dy <= 65535 && dz <= 65535 && band > 0.f);
  SGNN_CHECK_ARG(sdf && bricks);
  const int nbx = (dx + BRICK - 1) / BRICK, nby = (dy + BRICK - 1) / BRICK, nbz = (dz + BRICK - 1) / BRICK;
  SGNN_LAUNCH(k_raycast_bricks, dim3((nbx + 7) / 8, (nby + 3) / 4, nbz), dim3(256), 0, (hipStream_t)stream, sdf, dx, dy,
              dz, nbx, nby, band, bricks);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

namespace {

// the launches of the three forward entry points; COLOR: colors (dense R, G, B, A words) is read and rgba written;
// DIFF: the recording cast of section U, which has no normals, colours or counters
template <bool COLOR, bool DIFF>
int cast(const float *sdf, int dx, int dy, int dz, float band, const uint8_t *bricks, const sgnn_raycast_frame *frames,
         int nframes, int chunk, int h, int w, float depth_min, float dt, int nsamples, float *depth, float *normal,
         int64_t *counters, const uint8_t *colors, uint8_t *rgba, const Diff &D, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && dz >= 1 && dx <= 65535 && dy <= 65535 && dz <= 65535 && band > 0.f);
  SGNN_CHECK_ARG(nframes >= 0 && h >= 1 && w >= 1 && (int64_t)nframes * h * w < ((int64_t)1 << 31));
  SGNN_CHECK_ARG(dt > 0.f && nsamples >= 1 && nsamples <= (1 << 20));
  SGNN_CHECK_ARG(!DIFF || (D.features ? D.channels >= 1 && D.channels <= 16 : D.channels == 0));
  if (nframes == 0) return SGNN_OK;
  SGNN_CHECK_ARG(sdf && frames && depth);
  SGNN_CHECK_ARG(!COLOR || (colors && rgba && (((uintptr_t)colors | (uintptr_t)rgba) & 3) == 0));
  SGNN_CHECK_ARG(!DIFF || (D.hit && D.ok && !D.features == !D.feat));
  const dim3 tiles((w + 15) / 16, (h + 15) / 16);
  SGNN_CHECK_ARG(tiles.y <= 65535);
  if (chunk <= 0 || chunk > nframes) chunk = nframes;
  if (chunk > 65535) chunk = 65535;
  const Volume V{sdf, dx, dy, dz, band};
  const int nbx = (dx + BRICK - 1) / BRICK, nby = (dy + BRICK - 1) / BRICK;
  unsigned long long *ctr = reinterpret_cast<unsigned long long *>(counters);
  const uint32_t *cw = reinterpret_cast<const uint32_t *>(colors);
  uint32_t *pw = reinterpret_cast<uint32_t *>(rgba);
  hipStream_t s = (hipStream_t)stream;
  for (int f0 = 0; f0 < nframes; f0 += chunk) {
    const int f1 = f0 + chunk < nframes ? f0 + chunk : nframes;
    const dim3 grid(tiles.x, tiles.y, f1 - f0);
    if (!DIFF && bricks && normal)
      SGNN_LAUNCH((k_raycast<true, !DIFF, COLOR, DIFF>), grid, dim3(256), 0, s, V, bricks, nbx, nby, frames, f0, h, w,
                  depth_min, dt, nsamples, depth, normal, ctr, cw, pw, D);
    else if (bricks)
      SGNN_LAUNCH((k_raycast<true, false, COLOR, DIFF>), grid, dim3(256), 0, s, V, bricks, nbx, nby, frames, f0, h, w,
                  depth_min, dt, nsamples, depth, normal, ctr, cw, pw, D);
    else if (!DIFF && normal)
      SGNN_LAUNCH((k_raycast<false, !DIFF, COLOR, DIFF>), grid, dim3(256), 0, s, V, bricks, nbx, nby, frames, f0, h, w,
                  depth_min, dt, nsamples, depth, normal, ctr, cw, pw, D);
    else
      SGNN_LAUNCH((k_raycast<false, false, COLOR, DIFF>), grid, dim3(256), 0, s, V, bricks, nbx, nby, frames, f0, h, w,
                  depth_min, dt, nsamples, depth, normal, ctr, cw, pw, D);
    SGNN_CHECK_LAUNCH();
  }
  return SGNN_OK;
}

}  // namespace

SGNN_EXPORT int sgnn_raycast_cast(const float *sdf, int dx, int dy, int dz, float band, const uint8_t *bricks,
                                  const sgnn_raycast_frame *frames, int nframes, int chunk, int h, int w,
                                  float depth_min, float dt, int nsamples, float *depth, float *normal,
                                  int64_t *counters, sgnn_stream_t stream) {
  return cast<false, false>(sdf, dx, dy, dz, band, bricks, frames, nframes, chunk, h, w, depth_min, dt, nsamples, depth,
                     normal, counters, nullptr, nullptr, Diff{}, stream);
}

SGNN_EXPORT int sgnn_raycol_cast(const float *sdf, int dx, int dy, int dz, float band, const uint8_t *bricks,
                                 const sgnn_raycast_frame *frames, int nframes, int chunk, int h, int w,
                                 float depth_min, float dt, int nsamples, float *depth, float *normal,
                                 int64_t *counters, const uint8_t *colors, uint8_t *rgba, sgnn_stream_t stream) {
  return cast<true, false>(sdf, dx, dy, dz, band, bricks, frames, nframes, chunk, h, w, depth_min, dt, nsamples, depth,
                    normal, counters, colors, rgba, Diff{}, stream);
}

SGNN_EXPORT int sgnn_raygrad_cast(const float *sdf, int dx, int dy, int dz, float band, const uint8_t *bricks,
                                  const sgnn_raycast_frame *frames, int nframes, int chunk, int h, int w,
                                  float depth_min, float dt, int nsamples, const float *features, int channels,
                                  float *depth, int32_t *hit, float *feat, uint8_t *ok, sgnn_stream_t stream) {
  return cast<false, true>(sdf, dx, dy, dz, band, bricks, frames, nframes, chunk, h, w, depth_min, dt, nsamples, depth,
                           nullptr, nullptr, nullptr, nullptr, Diff{features, channels, hit, feat, ok}, stream);
}

SGNN_EXPORT int sgnn_raygrad_backward(const float *sdf, int dx, int dy, int dz, const sgnn_raycast_frame *frames,
                                      int nframes, int chunk, int h, int w, float depth_min, float dt, int nsamples,
                                      const int32_t *hit, const float *features, int channels,
                                      const float *grad_depth, const float *grad_feat, float *grad_sdf,
                                      float *grad_features, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && dz >= 1 && dx <= 65535 && dy <= 65535 && dz <= 65535);
  SGNN_CHECK_ARG(nframes >= 0 && h >= 1 && w >= 1 && (int64_t)nframes * h * w < ((int64_t)1 << 31));
  SGNN_CHECK_ARG(dt > 0.f && nsamples >= 1 && nsamples <= (1 << 20));
  SGNN_CHECK_ARG(features ? channels >= 1 && channels <= 16 : channels == 0);
  SGNN_CHECK_ARG(features || (!grad_feat && !grad_features));
  if (nframes == 0) return SGNN_OK;
  SGNN_CHECK_ARG(sdf && frames && hit);
  const dim3 tiles((w + 15) / 16, (h + 15) / 16);
  SGNN_CHECK_ARG(tiles.y <= 65535);
  if (!grad_sdf && !(grad_feat && grad_features)) return SGNN_OK;   // nothing to add to
  if (chunk <= 0 || chunk > nframes) chunk = nframes;
  if (chunk > 65535) chunk = 65535;
  const Volume V{sdf, dx, dy, dz, INFINITY};
  for (int f0 = 0; f0 < nframes; f0 += chunk) {
    const int f1 = f0 + chunk < nframes ? f0 + chunk : nframes;
    SGNN_LAUNCH(k_raycast_grad, dim3(tiles.x, tiles.y, f1 - f0), dim3(256), 0, (hipStream_t)stream, V, frames, f0, h, w,
                depth_min, dt, nsamples, hit, features, channels, grad_depth, grad_feat, grad_sdf, grad_features);
    SGNN_CHECK_LAUNCH();
  }
  return SGNN_OK;
}
