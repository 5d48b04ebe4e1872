// The per-voxel state of a TSDF volume (sdf, weight, free counter, 8.8 colour record) and the rules every entrance to a
// volume shares: fusion.hip (depth frames), points.hip (point clouds) and regrid.hip (resample / merge).  INTEGRATION.md
// sections D, M, P and Q are the contract; this header is the one place their common expressions are written, so the
// restatements of the tests hold all three files to the same bits.  The affine maps and finite_f live in geom.h.
// No kernels here.  Every includer is built with -ffp-contract=off: each product and sum below is rounded on its own.
#pragma once
#include "geom.h"

// ---- the oriented box outside of which a volume is never updated (voxel coordinates) ----------------------------------
struct TsdfObb {
  int on;
  float a[3];      // corner
  float e[3][3];   // edge vectors
  float ee[3];     // dot(e_k, e_k), formed on the host in the same order as below
};

// 0 <= dot(q - a, e_k) <= dot(e_k, e_k) for k = 0, 1, 2; dot in the order (x*x' + y*y') + z*z'
__device__ __forceinline__ bool tsdf_obb_contains(const TsdfObb &o, float qx, float qy, float qz) {
  const float rx = qx - o.a[0], ry = qy - o.a[1], rz = qz - o.a[2];
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float d = (rx * o.e[k][0] + ry * o.e[k][1]) + rz * o.e[k][2];
    in = in && d >= 0.f && d <= o.ee[k];
  }
  return in;
}

// obb12: a, e0, e1, e2; NULL: no box (on = 0)
static inline TsdfObb tsdf_obb_arg(const float *obb12) {
  TsdfObb o{};
  if (obb12) {
    o.on = 1;
    for (int c = 0; c < 3; ++c) o.a[c] = obb12[c];
    for (int k = 0; k < 3; ++k) {
      for (int c = 0; c < 3; ++c) o.e[k][c] = obb12[3 + 3 * k + c];
      o.ee[k] = (o.e[k][0] * o.e[k][0] + o.e[k][1] * o.e[k][1]) + o.e[k][2] * o.e[k][2];
    }
  }
  return o;
}

// ---- the state of one volume; color is NULL where the volume (or the call) carries none -------------------------------
struct TsdfVol {
  float *sdf;
  uint8_t *weight;
  int32_t *freec;
  uint2 *color;
};

// 0: a geometry pointer is NULL or the colour record is not 8-byte aligned.  The pointers come in const so that a volume
// a kernel only reads (regrid's source) takes the same road.
static inline int tsdf_vol_arg(const float *sdf, const uint8_t *weight, const int32_t *free_ctr, const uint16_t *color,
                               TsdfVol &v) {
  if (!sdf || !weight || !free_ctr || ((uintptr_t)color & 7) != 0) return 0;
  v = TsdfVol{const_cast<float *>(sdf), const_cast<uint8_t *>(weight), const_cast<int32_t *>(free_ctr),
              reinterpret_cast<uint2 *>(const_cast<uint16_t *>(color))};
  return 1;
}

// ---- one observation at range d (rules D.4, D.5) ---------------------------------------------------------------------
__device__ __forceinline__ float tsdf_trunc(float vs, float d) { return vs * 3.0f + d * vs; }

// sd0 > -trunc is the caller's test; the clamp to [-trunc, trunc]
__device__ __forceinline__ float tsdf_clamp_sd(float sd0, float trunc) {
  return sd0 >= 0.f ? fminf(trunc, sd0) : fmaxf(-trunc, sd0);
}

// the weight of an observation, a ramp fixed to 0.4 .. 4.0 m; the integer weight is (int) of it
__device__ __forceinline__ float tsdf_ramp(float d) {
  return fmaxf(4.5f * (1.0f - __fdiv_rn(d - 0.4f, 4.0f - 0.4f)), 1.0f);
}

// ---- the colour record: four 16-bit fields, R, G, B in 8.8 fixed point and the colour weight (section M) --------------
struct TsdfColor { uint32_t q[3], w; };

__device__ __forceinline__ TsdfColor tsdf_color_unpack(uint2 c) {
  return TsdfColor{{c.x & 0xFFFFu, c.x >> 16, c.y & 0xFFFFu}, c.y >> 16};
}

__device__ __forceinline__ uint2 tsdf_color_pack(uint32_t r, uint32_t g, uint32_t b, uint32_t w) {
  return make_uint2(r | g << 16, b | w << 16);
}

// an 8.8 field as a byte, halves up
__device__ __forceinline__ uint32_t tsdf_color8(uint32_t field) { return (field + 128u) >> 8; }

// ---- the once-per-call fold of points (section P) and merge (rule Q.8): the call is one observation of voxel v --------
// Each returns before any load or store where its weight (or count) is 0.
__device__ __forceinline__ void tsdf_fold_free(const TsdfVol &vol, int64_t v, uint32_t fc) {
  if (fc) vol.freec[v] = (int32_t)((uint32_t)vol.freec[v] + fc);          // wraps as uint32
}

// obs with weight wu (1 .. 255) into the running mean; sdf[v] is read only where the old weight is not 0
__device__ __forceinline__ void tsdf_fold_geometry(const TsdfVol &vol, int64_t v, float obs, int wu) {
  if (wu == 0) return;
  const int w = vol.weight[v];
  if (w != 0) obs = __fdiv_rn(vol.sdf[v] * (float)w + obs * (float)wu, (float)w + (float)wu);
  vol.sdf[v] = obs;
  vol.weight[v] = (uint8_t)min(w + wu, 255);
}

// ci (8.8) with weight wcu (1 .. 255) into the record, in integers, halves up
__device__ __forceinline__ void tsdf_fold_color(const TsdfVol &vol, int64_t v, const uint32_t (&ci)[3], uint32_t wcu) {
  if (wcu == 0) return;
  TsdfColor c = tsdf_color_unpack(vol.color[v]);
#pragma unroll
  for (int k = 0; k < 3; ++k) c.q[k] = c.w == 0 ? ci[k] : (c.q[k] * c.w + ci[k] * wcu + (c.w + wcu) / 2) / (c.w + wcu);
  vol.color[v] = tsdf_color_pack(c.q[0], c.q[1], c.q[2], min(c.w + wcu, 255u));
}
