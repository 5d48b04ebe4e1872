// Point clouds with known sensor origins fused into a scan volume (sgnn_amd.points): the third entrance next to depth
// frames (fusion.hip) and triangle meshes (voxelize.hip).  The rules are INTEGRATION.md section P; the project this one
// was modelled on has no counterpart, so that text is the contract, and tests/points_ref.py restates it independently in
// NumPy with plain Python integers for the accumulators.
//
// A ray o -> p is sampled every half voxel; every sample names a voxel, and that voxel's centre is projected back on
// the ray for a signed distance.  With carving a ray has hundreds of samples, without it a dozen, so a lane never owns
// a ray: the work is flattened.
//   k_points_count   one lane per ray: N samples (0 for a ray that is ignored or whose padded segment box misses the grid)
//                    and the grid box the call's segments can touch (wave min / max, then six atomics per wave)
//   (exclusive scan of N on the caller's side)
//   k_points_walk    one lane per SAMPLE.  A workgroup takes 256 consecutive samples; two lanes find the rays of the
//                    first and the last of them in the scanned offsets, every lane then searches only between those
//                    two, which is one or two rays with carving.  The lane forms its voxel, recomputes the voxel of
//                    sample n-1 for the duplicate test, and adds to integer accumulators with global atomics: one 64-bit
//                    add for the fixed-point sdf sum, one 64-bit add for (free count << 32 | weight), four more for a
//                    colour.  Integer sums do not depend on the arrival order: the result has no run-to-run noise.
//   k_points_fold    one lane per voxel of the box: accumulators -> the volume's running mean, once per call: the fold
//                    of tsdf.h, as regrid.hip's merge (tsdf.h: also fusion.hip's OBB test and rule D.5; geom.h: the affine map)
// The accumulators cover the box only: 16 bytes per box voxel, 48 with colour.
//
// Built with -ffp-contract=off (Makefile): every product and sum below is rounded on its own.
#include <math.h>
#include "common.h"
#include "tsdf.h"

namespace {

struct PtsBox {
  int lo[3], n[3];   // first voxel and extent per axis (x, y, z)
};

struct PtsGrid {
  int dx, dy, dz;
  float vs, dmin, dmax;
  int carve;
};

struct PtsRay {
  float o[3], dir[3];
  float d, trunc, t0, te;
  int wi, n;
};

constexpr float PTS_MAX_SAMPLES = 16777216.0f;      // (float)n is exact below 2^24

// rules P.1 - P.5 up to the sample count; false = the ray is ignored
__device__ __forceinline__ bool pts_ray(const float *__restrict__ points, const float *__restrict__ origins,
                                        const int32_t *__restrict__ origin_id, int64_t r, int norigins,
                                        const PtsGrid &g, PtsRay &R, bool &bad_id) {
  const int id = origin_id ? origin_id[r] : 0;
  R.n = 0;
  if (id < 0 || id >= norigins) {
    bad_id = true;
    return false;
  }
  const float px = points[3 * r], py = points[3 * r + 1], pz = points[3 * r + 2];
  R.o[0] = origins[3 * id];
  R.o[1] = origins[3 * id + 1];
  R.o[2] = origins[3 * id + 2];
  if (!(isfinite(px) && isfinite(py) && isfinite(pz) && isfinite(R.o[0]) && isfinite(R.o[1]) && isfinite(R.o[2])))
    return false;
  const float vx = px - R.o[0], vy = py - R.o[1], vz = pz - R.o[2];
  const float d = (float)sqrt((double)((vx * vx + vy * vy) + vz * vz));   // correctly rounded (the fp32 root is not)
  if (!(d > 0.f && d >= g.dmin && d <= g.dmax && isfinite(d))) return false;
  R.d = d;
  R.dir[0] = __fdiv_rn(vx, d);
  R.dir[1] = __fdiv_rn(vy, d);
  R.dir[2] = __fdiv_rn(vz, d);
  R.trunc = tsdf_trunc(g.vs, d);
  R.wi = (int)tsdf_ramp(d);
  R.t0 = g.carve ? g.dmin : fmaxf(d - R.trunc, 0.f);
  R.te = d + R.trunc;
  const float nf = floorf(__fdiv_rn(R.te - R.t0, g.vs * 0.5f));
  if (!(nf >= 0.f && nf < PTS_MAX_SAMPLES)) return false;
  R.n = (int)nf + 1;
  return true;
}

// the voxel of sample n as three integer-valued floats (NaN / inf possible: they fail the grid test)
__device__ __forceinline__ void pts_sample_voxel(const PtsRay &R, const TsdfAffine &w2g, float half, int n,
                                                 float (&v)[3]) {
  const float t = R.t0 + (float)n * half;
  float gq[3];
  tsdf_affine(w2g.m, R.o[0] + R.dir[0] * t, R.o[1] + R.dir[1] * t, R.o[2] + R.dir[2] * t, gq);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = roundf(gq[c]);
}

__global__ void k_points_box_init(int32_t *box) {
  if (threadIdx.x < 8) box[threadIdx.x] = threadIdx.x < 6 ? ((threadIdx.x & 1) ? INT32_MIN : INT32_MAX) : 0;
}

// counts[r] = N of ray r; box[0..5] = x0, x1, y0, y1, z0, z1 (inclusive) over the rays that can touch the grid;
// box[6] |= 1 when an origin id is out of range
__global__ __launch_bounds__(256) void k_points_count(const float *__restrict__ points,
                                                     const float *__restrict__ origins,
                                                     const int32_t *__restrict__ origin_id, int64_t nrays,
                                                     int norigins, TsdfAffine w2g, PtsGrid g,
                                                     int32_t *__restrict__ counts, int32_t *__restrict__ box) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int dims[3] = {g.dx, g.dy, g.dz};
  int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  bool bad_id = false;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < nrays; r += stride) {
    PtsRay R;
    int n = 0;
    if (pts_ray(points, origins, origin_id, r, norigins, g, R, bad_id)) {
      float a[3], b[3];
      tsdf_affine(w2g.m, R.o[0] + R.dir[0] * R.t0, R.o[1] + R.dir[1] * R.t0, R.o[2] + R.dir[2] * R.t0, a);
      tsdf_affine(w2g.m, R.o[0] + R.dir[0] * R.te, R.o[1] + R.dir[1] * R.te, R.o[2] + R.dir[2] * R.te, b);
      int l[3], h[3];
      bool hits = true;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float mn = fminf(a[c], b[c]), mx = fmaxf(a[c], b[c]);
        if (isfinite(a[c]) && isfinite(b[c])) {
          // one voxel of padding: half a voxel for the rounding of a sample, the rest for the fp32 error of the walk
          l[c] = (int)fminf(fmaxf(floorf(mn) - 1.0f, 0.f), (float)dims[c]);
          h[c] = (int)fmaxf(fminf(ceilf(mx) + 1.0f, (float)(dims[c] - 1)), -1.0f);
        } else {
          l[c] = 0;
          h[c] = dims[c] - 1;
        }
        hits = hits && l[c] <= h[c];
      }
      if (hits) {
        n = R.n;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          lo[c] = min(lo[c], l[c]);
          hi[c] = max(hi[c], h[c]);
        }
      }
    }
    counts[r] = n;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    for (int s = 32; s > 0; s >>= 1) {
      lo[c] = min(lo[c], __shfl_xor(lo[c], s));
      hi[c] = max(hi[c], __shfl_xor(hi[c], s));
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (lo[c] <= hi[c]) {
        atomicMin(&box[2 * c], lo[c]);
        atomicMax(&box[2 * c + 1], hi[c]);
      }
    }
  }
  if (bad_id) atomicOr(&box[6], 1);
}

// the last index q in [lo, hi] with offsets[q] <= s (offsets[lo] <= s is given)
__device__ __forceinline__ int64_t pts_find(const int64_t *__restrict__ offsets, int64_t lo, int64_t hi, int64_t s) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (offsets[mid] <= s) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// offsets: (nrays + 1) exclusive scan of counts.  acc_s / acc_wf: one int64 / uint64 per box voxel; acc_c: four
// uint64 per box voxel (sum R wi, sum G wi, sum B wi, sum wi) or NULL.
template <bool COLOR>
__global__ __launch_bounds__(256) void k_points_walk(const float *__restrict__ points,
                                                    const float *__restrict__ origins,
                                                    const int32_t *__restrict__ origin_id,
                                                    const uint8_t *__restrict__ colors, int channels, int64_t nrays,
                                                    int norigins, const int64_t *__restrict__ offsets, TsdfAffine w2g,
                                                    TsdfAffine g2w, TsdfObb obb, PtsGrid g, PtsBox box,
                                                    unsigned long long *__restrict__ acc_s,
                                                    unsigned long long *__restrict__ acc_wf,
                                                    unsigned long long *__restrict__ acc_c) {
  __shared__ int64_t span[2];
  const int64_t total = offsets[nrays];
  const int64_t ntiles = (total + 255) / 256;
  const float half = g.vs * 0.5f;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t s0 = tile * 256, s1 = min(s0 + 255, total - 1);
    if (threadIdx.x < 2) span[threadIdx.x] = pts_find(offsets, 0, nrays - 1, threadIdx.x ? s1 : s0);
    __syncthreads();
    const int64_t r_lo = span[0], r_hi = span[1];
    __syncthreads();
    const int64_t s = s0 + threadIdx.x;
    if (s > s1) continue;
    const int64_t r = pts_find(offsets, r_lo, r_hi, s);
    const int n = (int)(s - offsets[r]);
    PtsRay R;
    bool bad_id = false;
    if (!pts_ray(points, origins, origin_id, r, norigins, g, R, bad_id) || n >= R.n) continue;   // never: counts came from pts_ray
    float v[3];
    pts_sample_voxel(R, w2g, half, n, v);
    if (!(v[0] >= 0.f && v[0] < (float)g.dx && v[1] >= 0.f && v[1] < (float)g.dy && v[2] >= 0.f && v[2] < (float)g.dz))
      continue;
    if (obb.on && !tsdf_obb_contains(obb, v[0], v[1], v[2])) continue;
    if (n > 0) {
      float u[3];
      pts_sample_voxel(R, w2g, half, n - 1, u);
      if (u[0] == v[0] && u[1] == v[1] && u[2] == v[2]) continue;
    }
    // the accumulators exist for the box only; a voxel of the grid that the padded box misses cannot be reached
    // (k_points_count), and this test keeps the adds inside the allocation whatever the input
    const int bi = (int)v[0] - box.lo[0], bj = (int)v[1] - box.lo[1], bk = (int)v[2] - box.lo[2];
    if (bi < 0 || bi >= box.n[0] || bj < 0 || bj >= box.n[1] || bk < 0 || bk >= box.n[2]) continue;
    const int64_t idx = ((int64_t)bk * box.n[1] + bj) * box.n[0] + bi;
    float c[3];
    tsdf_affine(g2w.m, v[0], v[1], v[2], c);
    const float pz = ((c[0] - R.o[0]) * R.dir[0] + (c[1] - R.o[1]) * R.dir[1]) + (c[2] - R.o[2]) * R.dir[2];
    unsigned long long wf = pz < R.d ? (1ull << 32) : 0ull;
    const float sd0 = R.d - pz;
    if (sd0 > -R.trunc) {
      const int q = (int)roundf(__fdiv_rn(tsdf_clamp_sd(sd0, R.trunc), g.vs) * 4096.0f);
      atomicAdd(&acc_s[idx], (unsigned long long)((long long)q * R.wi));     // two's complement: a signed sum
      wf += (unsigned long long)R.wi;
      if constexpr (COLOR) {
        if (sd0 < R.trunc) {                                                  // free space gets no colour (section M)
          const uint8_t *px = colors + r * channels;
          if (channels == 3 || px[3] != 0) {
            unsigned long long *a = acc_c + 4 * idx;
            atomicAdd(&a[0], (unsigned long long)(px[0] * R.wi));
            atomicAdd(&a[1], (unsigned long long)(px[1] * R.wi));
            atomicAdd(&a[2], (unsigned long long)(px[2] * R.wi));
            atomicAdd(&a[3], (unsigned long long)R.wi);
          }
        }
      }
    }
    if (wf) atomicAdd(&acc_wf[idx], wf);
  }
}

template <bool COLOR>
__global__ __launch_bounds__(256) void k_points_fold(float *__restrict__ sdf, uint8_t *__restrict__ weight,
                                                    int32_t *__restrict__ freec, uint2 *__restrict__ color, int dx,
                                                    int dy, float vs, PtsBox box, const long long *__restrict__ acc_s,
                                                    const unsigned long long *__restrict__ acc_wf,
                                                    const unsigned long long *__restrict__ acc_c) {
  const TsdfVol vol{sdf, weight, freec, color};
  const int64_t nb = (int64_t)box.n[0] * box.n[1] * box.n[2];
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < nb; b += stride) {
    const unsigned long long wf = acc_wf[b];
    const int64_t row = b / box.n[0];
    const int i = box.lo[0] + (int)(b - row * box.n[0]);
    const int j = box.lo[1] + (int)(row % box.n[1]), k = box.lo[2] + (int)(row / box.n[1]);
    const int64_t v = ((int64_t)k * dy + j) * dx + i;
    const uint32_t W = (uint32_t)wf;
    tsdf_fold_free(vol, v, (uint32_t)(wf >> 32));
    if (W) tsdf_fold_geometry(vol, v, (float)((double)acc_s[b] / ((double)W * 4096.0)) * vs, (int)min(W, 255u));
    if constexpr (COLOR) {
      const unsigned long long cw = acc_c[4 * b + 3];
      if (cw) {
        uint32_t ci[3];                                                                // the call's mean, 8.8
#pragma unroll
        for (int c = 0; c < 3; ++c) ci[c] = (uint32_t)((256ull * acc_c[4 * b + c] + cw / 2) / cw);
        tsdf_fold_color(vol, v, ci, (uint32_t)(cw < 255ull ? cw : 255ull));
      }
    }
  }
}

int pts_box_arg(const int32_t *b, int dx, int dy, int dz, PtsBox &box) {
  const int dims[3] = {dx, dy, dz};
  for (int c = 0; c < 3; ++c) {
    if (b[2 * c] < 0 || b[2 * c + 1] >= dims[c] || b[2 * c] > b[2 * c + 1]) return 0;
    box.lo[c] = b[2 * c];
    box.n[c] = b[2 * c + 1] - b[2 * c] + 1;
  }
  return 1;
}

}  // namespace

SGNN_EXPORT int sgnn_points_count(const float *points, const float *origins, const int32_t *origin_id, int64_t nrays,
                                  int norigins, const float *world2grid, int dx, int dy, int dz, float voxel_size,
                                  float depth_min, float depth_max, int carve, int32_t *counts, int32_t *box,
                                  sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nrays >= 0 && nrays <= SGNN_POINTS_MAX_RAYS && norigins >= 1 && dx >= 1 && dy >= 1 && dz >= 1);
  SGNN_CHECK_ARG(voxel_size > 0.f && depth_max >= depth_min && isfinite(depth_max) && isfinite(depth_min));
  SGNN_CHECK_ARG(box && world2grid);
  TsdfAffine w2g;
  SGNN_CHECK_ARG(tsdf_affine_arg(world2grid, w2g));
  SGNN_LAUNCH(k_points_box_init, dim3(1), dim3(64), 0, (hipStream_t)stream, box);
  SGNN_CHECK_LAUNCH();
  if (nrays == 0) return SGNN_OK;
  SGNN_CHECK_ARG(points && origins && counts);
  const PtsGrid g{dx, dy, dz, voxel_size, depth_min, depth_max, carve != 0};
  SGNN_LAUNCH(k_points_count, dim3(sgnn_grid_for(nrays, 256, 8192)), dim3(256), 0, (hipStream_t)stream, points,
              origins, origin_id, nrays, norigins, w2g, g, counts, box);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_points_walk(const float *points, const float *origins, const int32_t *origin_id,
                                 const uint8_t *colors, int channels, int64_t nrays, int norigins,
                                 const int64_t *offsets, int64_t max_samples, const float *world2grid,
                                 const float *grid2world, const float *obb, int dx, int dy, int dz, float voxel_size,
                                 float depth_min, float depth_max, int carve, const int32_t *box, int64_t *acc_s,
                                 uint64_t *acc_wf, uint64_t *acc_c, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nrays >= 0 && nrays <= SGNN_POINTS_MAX_RAYS && norigins >= 1 && dx >= 1 && dy >= 1 && dz >= 1);
  SGNN_CHECK_ARG(voxel_size > 0.f && depth_max >= depth_min && isfinite(depth_max) && isfinite(depth_min));
  SGNN_CHECK_ARG(max_samples >= 0 && (colors == nullptr) == (acc_c == nullptr));
  SGNN_CHECK_ARG(colors == nullptr || channels == 3 || channels == 4);
  if (nrays == 0 || max_samples == 0) return SGNN_OK;
  SGNN_CHECK_ARG(points && origins && offsets && world2grid && grid2world && box && acc_s && acc_wf);
  SGNN_CHECK_ARG(((uintptr_t)acc_s & 7) == 0 && ((uintptr_t)acc_wf & 7) == 0 && ((uintptr_t)acc_c & 7) == 0);
  TsdfAffine w2g, g2w;
  PtsBox b;
  SGNN_CHECK_ARG(tsdf_affine_arg(world2grid, w2g) && tsdf_affine_arg(grid2world, g2w));
  SGNN_CHECK_ARG(pts_box_arg(box, dx, dy, dz, b));
  const TsdfObb o = tsdf_obb_arg(obb);
  const PtsGrid g{dx, dy, dz, voxel_size, depth_min, depth_max, carve != 0};
  // the number of samples is on the device (offsets[nrays]); max_samples, the caller's bound on it, only sizes the grid
  const dim3 grid(sgnn_grid_for(max_samples, 256, 8192));
  unsigned long long *s = reinterpret_cast<unsigned long long *>(acc_s);
  unsigned long long *wf = reinterpret_cast<unsigned long long *>(acc_wf);
  unsigned long long *c = reinterpret_cast<unsigned long long *>(acc_c);
  SGNN_LAUNCH(colors ? k_points_walk<true> : k_points_walk<false>, grid, dim3(256), 0, (hipStream_t)stream, points,
              origins, origin_id, colors, channels, nrays, norigins, offsets, w2g, g2w, o, g, b, s, wf, c);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_points_fold(float *sdf, uint8_t *weight, int32_t *free_ctr, uint16_t *color, int dx, int dy,
                                 int dz, float voxel_size, const int32_t *box, const int64_t *acc_s,
                                 const uint64_t *acc_wf, const uint64_t *acc_c, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && dz >= 1 && voxel_size > 0.f);
  TsdfVol vol;
  SGNN_CHECK_ARG(tsdf_vol_arg(sdf, weight, free_ctr, color, vol) && box && acc_s && acc_wf);
  SGNN_CHECK_ARG((color == nullptr) == (acc_c == nullptr));
  SGNN_CHECK_ARG(((uintptr_t)acc_s & 7) == 0 && ((uintptr_t)acc_wf & 7) == 0 && ((uintptr_t)acc_c & 7) == 0);
  PtsBox b;
  SGNN_CHECK_ARG(pts_box_arg(box, dx, dy, dz, b));
  const dim3 grid(sgnn_grid_for((int64_t)b.n[0] * b.n[1] * b.n[2], 256, 8192));
  const long long *s = reinterpret_cast<const long long *>(acc_s);
  const unsigned long long *wf = reinterpret_cast<const unsigned long long *>(acc_wf);
  const unsigned long long *c = reinterpret_cast<const unsigned long long *>(acc_c);
  SGNN_LAUNCH(color ? k_points_fold<true> : k_points_fold<false>, grid, dim3(256), 0, (hipStream_t)stream, vol.sdf,
              vol.weight, vol.freec, vol.color, dx, dy, voxel_size, b, s, wf, c);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
