// A TSDF volume's state moved to another grid (sgnn_amd.regrid): resample (store) and merge (fold).  The rules are
// INTEGRATION.md section Q; the project this one was modelled on has no counterpart, so that text is the contract, and
// tests/regrid_ref.py restates it independently in NumPy.
//
// One kernel text, k_regrid<COLOR, LINEAR, FOLD, SHAPE>, destination-major: one lane per destination voxel.  The lane
// maps its voxel through A (rows 0..2 of src.world2grid . inv(dst.world2grid), kernel arguments, wave-uniform) into
// source voxel coordinates, reads the nearest voxel or the participating corners of the cell, and either stores the
// result or folds it into the destination's running mean.  SHAPE is the destination brick of a wave: 4 x 4 x 4,
// 8 x 8 x 1 or 64 x 1 x 1.  Under a rotation a row of destination voxels is a slanted line in the source, and a brick
// keeps a wave's corner fetches in fewer cache lines; but every lane also stores 9 or 17 bytes to three or four arrays,
// and a brick breaks those stores into 16- and 32-byte pieces.  Measured (section Q, profiles/regrid_bench.json) the
// row wins by a third on a scene-sized volume, so the caller's default is 2; all three stay selectable.
//
// Block skip: the 8 corners of the block's destination box go through A; if their box, padded by one voxel and by a
// bound on the fp32 error of the map (RgMap::pad, formed on the host), misses the source grid on some axis, rules
// Q.3 - Q.6 fix every voxel of the block as unseen: store mode writes that, fold mode returns before any load.
// No LDS, no atomics, plain vector loads and stores; the colour record moves as one 8-byte access.  The volume's four
// pointers and the fold of rule Q.8 are those of tsdf.h, the affine row geom.h's: merge folds exactly as points.hip does.
//
// Built with -ffp-contract=off (Makefile): every product and sum below is rounded on its own.
#include <math.h>
#include "common.h"
#include "tsdf.h"

namespace {

struct RgMap {
  TsdfAffine A;   // rows 0..2 of A
  float pad[3];   // per source axis: 1 + a bound on the fp32 error of A.(i, j, k, 1) over the destination grid
};

struct RgDims {
  int x, y, z;
};

template <int SHAPE>
struct RgShape;
template <>
struct RgShape<0> {   // wave 4 x 4 x 4, block 8 x 8 x 4
  static constexpr int BX = 8, BY = 8, BZ = 4;
  static __device__ __forceinline__ void lane(int t, int &x, int &y, int &z) {
    const int l = t & 63, w = t >> 6;
    x = (l & 3) + 4 * (w & 1);
    y = ((l >> 2) & 3) + 4 * (w >> 1);
    z = l >> 4;
  }
};
template <>
struct RgShape<1> {   // wave 8 x 8 x 1, block 8 x 8 x 4
  static constexpr int BX = 8, BY = 8, BZ = 4;
  static __device__ __forceinline__ void lane(int t, int &x, int &y, int &z) {
    x = t & 7;
    y = (t >> 3) & 7;
    z = t >> 6;
  }
};
template <>
struct RgShape<2> {   // wave 64 x 1 x 1, block 64 x 4 x 1: the row-major baseline
  static constexpr int BX = 64, BY = 4, BZ = 1;
  static __device__ __forceinline__ void lane(int t, int &x, int &y, int &z) {
    x = t & 63;
    y = t >> 6;
    z = 0;
  }
};

// l(p, q, a) of rule Q.5; l(p, q, 0) = p by definition (p + 0 (q - p) would turn -0 into +0)
__device__ __forceinline__ float rg_lerp(float p, float q, float a) { return a == 0.f ? p : p + a * (q - p); }

// true: no voxel of the destination box [lo, hi] can see the source grid (the argument is in section Q, "Block skip")
__device__ __forceinline__ bool rg_block_misses(const RgMap &a, const RgDims &s, const int (&lo)[3],
                                                const int (&hi)[3]) {
  const float sd[3] = {(float)(s.x - 1), (float)(s.y - 1), (float)(s.z - 1)};
  bool miss = false;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    float mn = INFINITY, mx = -INFINITY;
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float g = tsdf_affine_row(a.A.m, r, (float)((c & 1) ? hi[0] : lo[0]), (float)((c & 2) ? hi[1] : lo[1]),
                                      (float)((c & 4) ? hi[2] : lo[2]));
      finite = finite && isfinite(g);
      mn = fminf(mn, g);
      mx = fmaxf(mx, g);
    }
    miss = miss || (finite && (mx + a.pad[r] < 0.f || mn - a.pad[r] > sd[r]));
  }
  return miss;
}

template <bool COLOR, bool LINEAR, bool FOLD, int SHAPE>
__global__ __launch_bounds__(256) void k_regrid(TsdfVol src, RgDims s, RgMap a, TsdfVol dst, RgDims d, int skip) {
  using S = RgShape<SHAPE>;
  int lx, ly, lz;
  S::lane(threadIdx.x, lx, ly, lz);
  const int bi = blockIdx.x * S::BX, bj = blockIdx.y * S::BY, bk = blockIdx.z * S::BZ;
  const int i = bi + lx, j = bj + ly, k = bk + lz;
  const bool inside = i < d.x && j < d.y && k < d.z;
  const int v = inside ? (k * d.y + j) * d.x + i : 0;   // < 2^31 inside: the volume's own limit; a tail lane forms none

  if (skip) {                                       // block-uniform
    const int lo[3] = {bi, bj, bk};
    const int hi[3] = {min(bi + S::BX, d.x) - 1, min(bj + S::BY, d.y) - 1, min(bk + S::BZ, d.z) - 1};
    if (rg_block_misses(a, s, lo, hi)) {
      if (!FOLD && inside) {
        dst.sdf[v] = -INFINITY;
        dst.weight[v] = 0;
        dst.freec[v] = 0;
        if (COLOR) dst.color[v] = make_uint2(0u, 0u);
      }
      return;
    }
  }
  if (!inside) return;

  // rule 1: the voxel's position in source voxel coordinates; rule 3: its nearest voxel
  const float fi = (float)i, fj = (float)j, fk = (float)k;
  float g[3];
  tsdf_affine(a.A.m, fi, fj, fk, g);
  const float sd[3] = {(float)(s.x - 1), (float)(s.y - 1), (float)(s.z - 1)};
  const float r[3] = {roundf(g[0]), roundf(g[1]), roundf(g[2])};
  const bool r_in = r[0] >= 0.f && r[0] <= sd[0] && r[1] >= 0.f && r[1] <= sd[1] && r[2] >= 0.f && r[2] <= sd[2];
  const int rv = r_in ? ((int)r[2] * s.y + (int)r[1]) * s.x + (int)r[0] : 0;

  float s2 = -INFINITY;
  int w2 = 0;
  bool valid = false;
  if (LINEAR) {
    // rule 5: the cell, and per axis one participating index where a == 0, else two
    const float f[3] = {floorf(g[0]), floorf(g[1]), floorf(g[2])};
    const float al[3] = {g[0] - f[0], g[1] - f[1], g[2] - f[2]};
    bool in = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) in = in && f[c] >= 0.f && (al[c] == 0.f ? f[c] : f[c] + 1.0f) <= sd[c];
    if (in) {
      const int base = ((int)f[2] * s.y + (int)f[1]) * s.x + (int)f[0];
      // a corner of zero weight is never read: its offset is 0, so the lane reads the participating one again
      const int ox = al[0] == 0.f ? 0 : 1, oy = al[1] == 0.f ? 0 : s.x, oz = al[2] == 0.f ? 0 : s.x * s.y;
      float p[8];
      int wmin = 255;
      bool seen = true;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int q = base + ((c & 1) ? ox : 0) + ((c & 2) ? oy : 0) + ((c & 4) ? oz : 0);
        p[c] = src.sdf[q];
        const int w = src.weight[q];
        wmin = min(wmin, w);
        seen = seen && w > 0 && isfinite(p[c]);     // rule 2
      }
      if (seen) {
        const float x00 = rg_lerp(p[0], p[1], al[0]), x10 = rg_lerp(p[2], p[3], al[0]);
        const float x01 = rg_lerp(p[4], p[5], al[0]), x11 = rg_lerp(p[6], p[7], al[0]);
        s2 = rg_lerp(rg_lerp(x00, x10, al[1]), rg_lerp(x01, x11, al[1]), al[2]);
        w2 = wmin;
        valid = true;                               // r participates, so r_in holds
      }
    }
  } else if (r_in) {
    // rule 4
    const float p = src.sdf[rv];
    const int w = src.weight[rv];
    if (w > 0 && isfinite(p)) {
      s2 = p;
      w2 = w;
      valid = true;
    }
  }
  const int32_t f2 = r_in ? src.freec[rv] : 0;      // rule 6
  uint2 c2 = make_uint2(0u, 0u);
  if (COLOR && valid) c2 = src.color[rv];

  if (!FOLD) {
    dst.sdf[v] = s2;
    dst.weight[v] = (uint8_t)w2;
    dst.freec[v] = f2;
    if (COLOR) dst.color[v] = c2;
    return;
  }
  // rule 8: the sample is one observation of the voxel; a sample that is not valid has w2 == 0 and no colour
  tsdf_fold_free(dst, v, (uint32_t)f2);
  tsdf_fold_geometry(dst, v, s2, w2);
  if (COLOR) {
    const TsdfColor c = tsdf_color_unpack(c2);
    tsdf_fold_color(dst, v, c.q, c.w);
  }
}

template <bool COLOR, bool LINEAR, bool FOLD, int SHAPE>
void rg_launch_shape(const TsdfVol &src, const RgDims &s, const RgMap &a, const TsdfVol &dst, const RgDims &d, int skip,
                     hipStream_t stream) {
  using S = RgShape<SHAPE>;
  const dim3 grid((d.x + S::BX - 1) / S::BX, (d.y + S::BY - 1) / S::BY, (d.z + S::BZ - 1) / S::BZ);
  SGNN_LAUNCH((k_regrid<COLOR, LINEAR, FOLD, SHAPE>), grid, dim3(256), 0, stream, src, s, a, dst, d, skip);
}

template <bool COLOR, bool LINEAR, bool FOLD>
void rg_launch_mode(int shape, const TsdfVol &src, const RgDims &s, const RgMap &a, const TsdfVol &dst, const RgDims &d,
                    int skip, hipStream_t stream) {
  if (shape == 0) rg_launch_shape<COLOR, LINEAR, FOLD, 0>(src, s, a, dst, d, skip, stream);
  else if (shape == 1) rg_launch_shape<COLOR, LINEAR, FOLD, 1>(src, s, a, dst, d, skip, stream);
  else rg_launch_shape<COLOR, LINEAR, FOLD, 2>(src, s, a, dst, d, skip, stream);
}

template <bool FOLD>
void rg_launch(bool color, bool linear, int shape, const TsdfVol &src, const RgDims &s, const RgMap &a, const TsdfVol &dst,
               const RgDims &d, int skip, hipStream_t stream) {
  if (color) {
    if (linear) rg_launch_mode<true, true, FOLD>(shape, src, s, a, dst, d, skip, stream);
    else rg_launch_mode<true, false, FOLD>(shape, src, s, a, dst, d, skip, stream);
  } else {
    if (linear) rg_launch_mode<false, true, FOLD>(shape, src, s, a, dst, d, skip, stream);
    else rg_launch_mode<false, false, FOLD>(shape, src, s, a, dst, d, skip, stream);
  }
}

bool rg_dims_ok(int x, int y, int z) {
  return x >= 1 && y >= 1 && z >= 1 && x <= 65535 && y <= 65535 && z <= 65535 && (int64_t)x * y * z < (1ll << 31);
}

// A and, per source axis, 1 + 16 ulp-halves of the largest sum of magnitudes the row can reach on the destination grid
int rg_map_arg(const float *host12, const RgDims &d, RgMap &a) {
  if (!tsdf_affine_arg(host12, a.A)) return 0;
  const float *m = a.A.m;
  for (int r = 0; r < 3; ++r) {
    const double sum = fabs((double)m[4 * r]) * (d.x - 1) + fabs((double)m[4 * r + 1]) * (d.y - 1) +
                       fabs((double)m[4 * r + 2]) * (d.z - 1) + fabs((double)m[4 * r + 3]);
    const double pad = 1.0 + 16.0 * sum * 5.9604644775390625e-08;   // 2^-24
    if (!(pad < 1e30)) return 0;
    a.pad[r] = (float)(pad * (1.0 + 1e-6));
  }
  return 1;
}

}  // namespace

// the one host side of both entry points; the two differ in the colour rule and the template argument only
static int regrid(bool fold, const float *src_sdf, const uint8_t *src_weight, const int32_t *src_free,
                  const uint16_t *src_color, int sdx, int sdy, int sdz, const float *map, int linear, int skip,
                  int shape, float *dst_sdf, uint8_t *dst_weight, int32_t *dst_free, uint16_t *dst_color, int ddx,
                  int ddy, int ddz, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(rg_dims_ok(sdx, sdy, sdz) && rg_dims_ok(ddx, ddy, ddz) && shape >= 0 && shape <= 2);
  TsdfVol src, dst;
  SGNN_CHECK_ARG(tsdf_vol_arg(src_sdf, src_weight, src_free, src_color, src) && map);
  SGNN_CHECK_ARG(tsdf_vol_arg(dst_sdf, dst_weight, dst_free, dst_color, dst));
  if (!fold) SGNN_CHECK_ARG((src_color == nullptr) == (dst_color == nullptr));   // store: colour on both or on neither
  SGNN_CHECK_ARG(dst_sdf != src_sdf && dst_weight != src_weight && dst_free != src_free);
  const RgDims s{sdx, sdy, sdz}, d{ddx, ddy, ddz};
  RgMap a;
  SGNN_CHECK_ARG(rg_map_arg(map, d, a));
  const bool color = src.color != nullptr && dst.color != nullptr;   // fold (rule 8): only where both volumes carry it
  if (!color) src.color = dst.color = nullptr;
  if (fold) rg_launch<true>(color, linear != 0, shape, src, s, a, dst, d, skip != 0, (hipStream_t)stream);
  else rg_launch<false>(color, linear != 0, shape, src, s, a, dst, d, skip != 0, (hipStream_t)stream);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_regrid_resample(const float *src_sdf, const uint8_t *src_weight, const int32_t *src_free,
                                     const uint16_t *src_color, int sdx, int sdy, int sdz, const float *map,
                                     int linear, int skip, int shape, float *dst_sdf, uint8_t *dst_weight,
                                     int32_t *dst_free, uint16_t *dst_color, int ddx, int ddy, int ddz,
                                     sgnn_stream_t stream) {
  return regrid(false, src_sdf, src_weight, src_free, src_color, sdx, sdy, sdz, map, linear, skip, shape, dst_sdf,
                dst_weight, dst_free, dst_color, ddx, ddy, ddz, stream);
}

SGNN_EXPORT int sgnn_regrid_merge(const float *src_sdf, const uint8_t *src_weight, const int32_t *src_free,
                                  const uint16_t *src_color, int sdx, int sdy, int sdz, const float *map, int linear,
                                  int skip, int shape, float *dst_sdf, uint8_t *dst_weight, int32_t *dst_free,
                                  uint16_t *dst_color, int ddx, int ddy, int ddz, sgnn_stream_t stream) {
  return regrid(true, src_sdf, src_weight, src_free, src_color, sdx, sdy, sdz, map, linear, skip, shape, dst_sdf,
                dst_weight, dst_free, dst_color, ddx, ddy, ddz, stream);
}
