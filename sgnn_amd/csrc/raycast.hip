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
#include "geom.h"

namespace {

constexpr int BRICK = 8;   // edge of a brick of the skip table

struct Volume {
  const float *sdf;
  int dx, dy, dz;
  float band;
};

// rule 4: the sample at grid position g; false = invalid
__device__ __forceinline__ bool sample(const Volume &V, float gx, float gy, float gz, float &v, GeomCell *cell = nullptr) {
  GeomCell c;
  float s[8];
  v = 0.f;
  if (!geom_cell(V.dx, V.dy, V.dz, gx, gy, gz, c)) return false;
  if (cell) *cell = c;
  geom_gather(V.sdf + c.base, V.dx, V.dy, s);
  const float b = V.band;                           // |c| < band is false for a NaN and for an infinity
  if (!(fabsf(s[0]) < b && fabsf(s[1]) < b && fabsf(s[2]) < b && fabsf(s[3]) < b && fabsf(s[4]) < b &&
        fabsf(s[5]) < b && fabsf(s[6]) < b && fabsf(s[7]) < b))
    return false;
  const float x00 = s[0] + c.a[0] * (s[1] - s[0]), x01 = s[2] + c.a[0] * (s[3] - s[2]);
  const float x10 = s[4] + c.a[0] * (s[5] - s[4]), x11 = s[6] + c.a[0] * (s[7] - s[6]);
  const float y0 = x00 + c.a[1] * (x01 - x00), y1 = x10 + c.a[1] * (x11 - x10);
  v = y0 + c.a[2] * (y1 - y0);
  return true;
}

// Section N: the colour at the hit g, from the cell's corners that have one (A != 0); the R, G, B, A bytes of the
// pixel as one word, 0 = no colour.  colors is the dense (dz, dy, dx) volume of R, G, B, A words.
__device__ __forceinline__ uint32_t hit_color(const Volume &V, const uint32_t *__restrict__ colors, float gx, float gy,
                                              float gz) {
  GeomCell cell;
  if (!geom_cell(V.dx, V.dy, V.dz, gx, gy, gz, cell)) return 0u;
  uint32_t c[8];
  geom_gather(colors + cell.base, V.dx, V.dy, c);
  const GeomWeights W(cell.a);
  float s = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    // a corner without a colour adds a weight of zero: the sums are those over the counted corners, bit for bit
    const float w = (c[i] >> 24) ? W.corner(i) : 0.f;
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

// the pixel of a lane: a block covers 16x16 pixels, each of its four waves an 8x8 tile
__device__ __forceinline__ void lane_pixel(int &i, int &j) {
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  i = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  j = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
}

// rule 2: the ray of pixel (i, j) of a frame; its direction is the pose's linear part of (cx, cy, 1)
__device__ __forceinline__ Ray pixel_ray(const sgnn_raycast_frame &F, int i, int j, float depth_min, float dt) {
  const float cx = geom_unproject(F.intr, 0, (float)i), cy = geom_unproject(F.intr, 1, (float)j);
  return Ray{F.g[3], F.g[7], F.g[11], geom_linear_row(F.g, 0, cx, cy, 1.0f), geom_linear_row(F.g, 1, cx, cy, 1.0f),
             geom_linear_row(F.g, 2, cx, cy, 1.0f), depth_min, dt};   // a product with 1 is exact
}

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
  int i, j;
  lane_pixel(i, j);
  const int f = f0 + (int)blockIdx.z;
  const sgnn_raycast_frame &F = frames[f];
  const float *G = F.g;
  const bool pixel = i < w && j < h;
  const bool live = pixel && G[0] == G[0];          // non-finite pose (the host stores NaN): the frame stays empty
  const Ray R = pixel_ray(F, i, j, depth_min, dt);
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
      float n[3] = {NAN, NAN, NAN};
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
          geom_unit(geom_linear_col(G, 0, a, b, c), geom_linear_col(G, 1, a, b, c), geom_linear_col(G, 2, a, b, c), n);
        }
      }
      normal[px * 3 + 0] = n[0];
      normal[px * 3 + 1] = n[1];
      normal[px * 3 + 2] = n[2];
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
      GeomCell c;
      const bool cell = has && geom_cell(V.dx, V.dy, V.dz, R.ox + hit * R.dx, R.oy + hit * R.dy, R.oz + hit * R.dz, c);
      bool ok = cell;
      if (cell) {
#pragma unroll
        for (int i = 0; i < 8; ++i) ok = (fabsf(V.sdf[c.base + geom_corner(V.dx, V.dy, i)]) < V.band) && ok;
      }
      D.ok[px] = ok ? 1 : 0;
      if (D.feat) {
        float wgt[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) wgt[i] = cell ? GeomWeights(c.a).corner(i) : 0.f;
        for (int ch = 0; ch < D.channels; ++ch) {
          float acc = 0.f;
          if (cell) {   // straight from the loads, corner by corner: a gather into registers first costs VGPRs here
            const float *p = D.features + c.base * D.channels + ch;
            acc = wgt[0] * p[0];
#pragma unroll
            for (int i = 1; i < 8; ++i) acc = acc + wgt[i] * p[geom_corner(V.dx, V.dy, i) * D.channels];
          }
          D.feat[px * D.channels + ch] = acc;
        }
      }
    }
  }
  if (counters) {                                   // kernel argument: the same for every lane
    const long long e = wave_sum(n_eval), s = wave_sum(n_skip);
    if ((threadIdx.x & 63) == 0) {                  // lane 0
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
  int i, j;
  lane_pixel(i, j);
  const int f = f0 + (int)blockIdx.z;
  if (!(i < w && j < h)) return;
  const sgnn_raycast_frame &F = frames[f];
  const int64_t px = ((int64_t)f * h + j) * w + i;
  const int k = hit[px];
  if (!(F.g[0] == F.g[0]) || k < 1 || k >= nsamples) return;   // no hit: the incoming gradient is not even read
  const Ray R = pixel_ray(F, i, j, depth_min, dt);               // rule H2
  // rules H3 and H4: both samples of the crossing; every finite corner counts, the forward found them usable
  const float t0 = R.t0 + (float)(k - 1) * R.dt, t1 = R.t0 + (float)k * R.dt;
  float pv, v;
  GeomCell c0, c1;                                    // V.band is infinite here
  if (!(sample(V, R.ox + t0 * R.dx, R.oy + t0 * R.dy, R.oz + t0 * R.dz, pv, &c0) &&
        sample(V, R.ox + t1 * R.dx, R.oy + t1 * R.dy, R.oz + t1 * R.dz, v, &c1)))
    return;
  const float den = pv - v;
  const float ts = t0 + dt * __fdiv_rn(pv, den);     // the forward's depth
  float Gs = grad_depth ? grad_depth[px] : 0.f;
  GeomCell cs;
  if (grad_feat && geom_cell(V.dx, V.dy, V.dz, R.ox + ts * R.dx, R.oy + ts * R.dy, R.oz + ts * R.dz, cs)) {
    const GeomWeights W(cs.a);
    for (int ch = 0; ch < channels; ++ch) {
      const float gf = grad_feat[px * channels + ch];
      const int64_t at = cs.base * channels + ch;
      float q[8];
      geom_gather(features + at, V.dx, V.dy, q, channels);
      // the gradient of rule 3's interpolant in its weight form (register.hip's rule 4 lerps and rounds differently)
      float qx = (W.z[0] * W.y[0]) * (q[1] - q[0]);
      qx = qx + (W.z[0] * W.y[1]) * (q[3] - q[2]);
      qx = qx + (W.z[1] * W.y[0]) * (q[5] - q[4]);
      qx = qx + (W.z[1] * W.y[1]) * (q[7] - q[6]);
      float qy = (W.z[0] * W.x[0]) * (q[2] - q[0]);
      qy = qy + (W.z[0] * W.x[1]) * (q[3] - q[1]);
      qy = qy + (W.z[1] * W.x[0]) * (q[6] - q[4]);
      qy = qy + (W.z[1] * W.x[1]) * (q[7] - q[5]);
      float qz = (W.y[0] * W.x[0]) * (q[4] - q[0]);
      qz = qz + (W.y[0] * W.x[1]) * (q[5] - q[1]);
      qz = qz + (W.y[1] * W.x[0]) * (q[6] - q[2]);
      qz = qz + (W.y[1] * W.x[1]) * (q[7] - q[3]);
      Gs = Gs + gf * ((qx * R.dx + qy * R.dy) + qz * R.dz);
      if (grad_features) {
#pragma unroll
        for (int c = 0; c < 8; ++c)
          atomicAdd(grad_features + at + geom_corner(V.dx, V.dy, c) * channels, gf * W.corner(c));
      }
    }
  }
  if (!grad_sdf) return;
  const float A = __fdiv_rn(Gs * dt, den * den);
  const float cpv = A * (-v), cv = A * pv;
#pragma unroll
  for (int c = 0; c < 8; ++c) atomicAdd(grad_sdf + c0.base + geom_corner(V.dx, V.dy, c), cpv * GeomWeights(c0.a).corner(c));
#pragma unroll
  for (int c = 0; c < 8; ++c) atomicAdd(grad_sdf + c1.base + geom_corner(V.dx, V.dy, c), cv * GeomWeights(c1.a).corner(c));
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

// what the forward entrances and the backward check alike; tiles: the 16x16 pixel blocks of a frame (no frames, no launch)
int frames_arg(int dx, int dy, int dz, int nframes, int h, int w, float dt, int nsamples, const float *features,
               int channels, dim3 &tiles) {
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && dz >= 1 && dx <= 65535 && dy <= 65535 && dz <= 65535);
  SGNN_CHECK_ARG(nframes >= 0 && h >= 1 && w >= 1 && (int64_t)nframes * h * w < ((int64_t)1 << 31));
  SGNN_CHECK_ARG(dt > 0.f && nsamples >= 1 && nsamples <= (1 << 20));
  SGNN_CHECK_ARG(features ? channels >= 1 && channels <= 16 : channels == 0);
  tiles = dim3((w + 15) / 16, (h + 15) / 16);
  SGNN_CHECK_ARG(nframes == 0 || tiles.y <= 65535);
  return SGNN_OK;
}

// launch(f0, n) for the frames f0 .. f0 + n - 1 of every chunk; a chunk is one launch and at most 65535 frames
template <typename L>
int for_frame_chunks(int nframes, int chunk, L launch) {
  if (chunk <= 0 || chunk > nframes) chunk = nframes;
  if (chunk > 65535) chunk = 65535;
  for (int f0 = 0; f0 < nframes; f0 += chunk) {
    launch(f0, (f0 + chunk < nframes ? f0 + chunk : nframes) - f0);
    SGNN_CHECK_LAUNCH();
  }
  return SGNN_OK;
}

// the launches of the three forward entry points; COLOR: colors (dense R, G, B, A words) is read and rgba written;
// DIFF: the recording cast of section U, which has no normals, colours or counters
template <bool COLOR, bool DIFF>
int cast(const float *sdf, int dx, int dy, int dz, float band, const uint8_t *bricks, const sgnn_raycast_frame *frames,
         int nframes, int chunk, int h, int w, float depth_min, float dt, int nsamples, float *depth, float *normal,
         int64_t *counters, const uint8_t *colors, uint8_t *rgba, const Diff &D, sgnn_stream_t stream) {
  dim3 tiles;
  if (const int rc = frames_arg(dx, dy, dz, nframes, h, w, dt, nsamples, D.features, D.channels, tiles)) return rc;
  SGNN_CHECK_ARG(band > 0.f);
  if (nframes == 0) return SGNN_OK;
  SGNN_CHECK_ARG(sdf && frames && depth);
  SGNN_CHECK_ARG(!COLOR || (colors && rgba && (((uintptr_t)colors | (uintptr_t)rgba) & 3) == 0));
  SGNN_CHECK_ARG(!DIFF || (D.hit && D.ok && !D.features == !D.feat));
  const Volume V{sdf, dx, dy, dz, band};
  const int nbx = (dx + BRICK - 1) / BRICK, nby = (dy + BRICK - 1) / BRICK;
  return for_frame_chunks(nframes, chunk, [&](int f0, int n) {
    auto go = [&](auto kernel) {
      SGNN_LAUNCH(kernel, dim3(tiles.x, tiles.y, n), dim3(256), 0, (hipStream_t)stream, V, bricks, nbx, nby, frames, f0,
                  h, w, depth_min, dt, nsamples, depth, normal, reinterpret_cast<unsigned long long *>(counters),
                  reinterpret_cast<const uint32_t *>(colors), reinterpret_cast<uint32_t *>(rgba), D);
    };
    if (!DIFF && bricks && normal) go(k_raycast<true, !DIFF, COLOR, DIFF>);
    else if (bricks) go(k_raycast<true, false, COLOR, DIFF>);
    else if (!DIFF && normal) go(k_raycast<false, !DIFF, COLOR, DIFF>);
    else go(k_raycast<false, false, COLOR, DIFF>);
  });
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
  dim3 tiles;
  if (const int rc = frames_arg(dx, dy, dz, nframes, h, w, dt, nsamples, features, channels, tiles)) return rc;
  SGNN_CHECK_ARG(features || (!grad_feat && !grad_features));
  if (nframes == 0) return SGNN_OK;
  SGNN_CHECK_ARG(sdf && frames && hit);
  if (!grad_sdf && !(grad_feat && grad_features)) return SGNN_OK;   // nothing to add to
  const Volume V{sdf, dx, dy, dz, INFINITY};
  return for_frame_chunks(nframes, chunk, [&](int f0, int n) {
    SGNN_LAUNCH(k_raycast_grad, dim3(tiles.x, tiles.y, n), dim3(256), 0, (hipStream_t)stream, V, frames, f0, h, w,
                depth_min, dt, nsamples, hit, features, channels, grad_depth, grad_feat, grad_sdf, grad_features);
  });
}
