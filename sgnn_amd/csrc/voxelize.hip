// Triangle meshes to signed distance volumes (sgnn_amd.voxelize): the exact signed distance of every voxel centre within
// a narrow band of a mesh.  The rules are listed in INTEGRATION.md section L; that text is the contract, and
// tests/voxelize_ref.py restates it independently in NumPy.
//
// Kernels:
//   k_vox_grid_coords  one thread per vertex: world -> grid coordinates (rule 1)
//   k_vox_bricks       one thread per face walks the 8x8x8 bricks its dilated box touches (its whole wave, if they are
//                      many): FILL = false counts them, FILL = true writes the face into the CSR lists (the scan between
//                      the two is the caller's)
//   k_vox_edges        one thread per usable face enters its three undirected edges into the first-member table
//   k_vox_normals      one thread per usable face adds its share to the vertex and edge pseudo-normals (rule 5):
//                      fp64 contributions quantised to int64, summed with integer atomics, so the order does not matter
//   k_vox_nearest      one workgroup per non-empty brick, two voxels per lane.  The brick's face records go through LDS in
//                      batches of SGNN_VOX_BATCH; every lane reads them as broadcasts, rejects a face whose dilated box
//                      does not hold its voxel, and keeps the best (d2, face) in registers (rule 3).  The tail takes the
//                      root, applies the band and signs the distance (rules 4 and 6).
//   k_vox_tsdf         one thread per voxel: signed voxels -> metres, -inf outside the band, and the weight
//
// Built with -ffp-contract=off (Makefile): distances and faces equal meshdist's bit for bit (tri_dist.h is shared).
#include <math.h>
#include "common.h"
#include "box_lists.h"  // the brick walk of k_vox_bricks, shared with meshdist.hip
#include "first_table.h"
#include "tri_dist.h"
#include "geom.h"       // the affine row of k_vox_grid_coords

namespace {

constexpr int BRICK = 8;                  // voxels per brick axis; 512 voxels, two per lane of a 256-thread workgroup
constexpr int BATCH = SGNN_VOX_BATCH;     // face records staged per round: 128 * (48 + 24 + 4) B = 9.5 KiB of LDS
constexpr double Q32 = 4294967296.0;      // 2^32: the fixed point of the pseudo-normal sums

// The voxel box of a face: its vertex box grown by band and a margin of 2^-16 of the largest magnitude involved, far
// above the rounding of rule 2 (section G: 2^-20 of it), so that no voxel whose computed distance is within the band
// lies outside.  An ignored face (box +inf, -inf) gets an empty box.
__device__ __forceinline__ void vox_box(const float *__restrict__ bx, float band, float dmax, float (&lo)[3],
                                        float (&hi)[3]) {
  const float inf = __int_as_float(0x7F800000);
  if (!(bx[0] <= bx[3])) {
    lo[0] = lo[1] = lo[2] = inf;
    hi[0] = hi[1] = hi[2] = -inf;
    return;
  }
  float m = fmaxf(band, dmax);
#pragma unroll
  for (int k = 0; k < 6; ++k) m = fmaxf(m, fabsf(bx[k]));
  const float marg = band + m * 1.52587890625e-05f;               // 2^-16
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = bx[k] - marg;
    hi[k] = bx[k + 3] + marg;
  }
}

// voxels [i0, i1] of an axis of n voxels with lo <= i <= hi; false if there is none
__device__ __forceinline__ bool vox_range(float lo, float hi, int n, int &i0, int &i1) {
  const float l = fmaxf(ceilf(lo), 0.f), h = fminf(floorf(hi), (float)(n - 1));
  if (!(l <= h)) return false;
  i0 = (int)l;
  i1 = (int)h;
  return true;
}

__global__ __launch_bounds__(256) void k_vox_grid_coords(const float *__restrict__ verts, int64_t nv, TsdfAffine w2g,
                                                        float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv) return;
  const float x = verts[i * 3], y = verts[i * 3 + 1], z = verts[i * 3 + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r) out[i * 3 + r] = tsdf_affine_row(w2g.m, r, x, y, z);
}

template <bool FILL>
__global__ __launch_bounds__(256) void k_vox_bricks(const float *__restrict__ boxes, int ntri, float band, int dx, int dy,
                                                   int dz, const int32_t *__restrict__ offsets,
                                                   int32_t *__restrict__ counts, int32_t *__restrict__ refs) {
  const int t = (int)(blockIdx.x * 256 + threadIdx.x);
  const int nbx = (dx + BRICK - 1) / BRICK, nby = (dy + BRICK - 1) / BRICK;
  CellRange r = {0, 0, 0, 0, 0, 0};                               // in bricks
  if (t < ntri) {
    float lo[3], hi[3];
    vox_box(boxes + (int64_t)t * 6, band, (float)max(dx, max(dy, dz)), lo, hi);
    int x1, y1, z1;
    if (vox_range(lo[0], hi[0], dx, r.x0, x1) && vox_range(lo[1], hi[1], dy, r.y0, y1) &&
        vox_range(lo[2], hi[2], dz, r.z0, z1)) {
      r.x0 /= BRICK, r.y0 /= BRICK, r.z0 /= BRICK;
      r.sx = x1 / BRICK - r.x0 + 1;
      r.sy = y1 / BRICK - r.y0 + 1;
      r.sz = z1 / BRICK - r.z0 + 1;
    }
  }
  list_in_cells<FILL>(r, t, nbx, nby, offsets, counts, refs);    // every lane: it holds a ballot
}

// the undirected edge (i, j) as a key; never all ones, since both are vertex indices below 2^31
__device__ __forceinline__ uint64_t edge_key(int i, int j) {
  return ((uint64_t)(uint32_t)min(i, j) << 32) | (uint64_t)(uint32_t)max(i, j);
}
__device__ __forceinline__ int64_t edge_home(uint64_t key, int64_t cap) {
  return (int64_t)(sgnn_hash64(key) % (uint64_t)cap);
}

__global__ __launch_bounds__(256) void k_vox_edges(const int32_t *__restrict__ faces, const uint8_t *__restrict__ usable,
                                                  int ntri, uint64_t *ekeys, int32_t *efirst, int64_t cap) {
  const int t = (int)(blockIdx.x * 256 + threadIdx.x);
  if (t >= ntri || !usable[t]) return;                            // a usable face has three indices in range
  const int32_t *fc = faces + (int64_t)t * 3;
  auto enter = [&](int i, int j) {
    const uint64_t key = edge_key(i, j);
    first_insert(ekeys, efirst, cap, edge_home(key, cap), (int32_t)t, key, [&](uint64_t q) { return q == key; });
  };
  enter(fc[0], fc[1]);
  enter(fc[1], fc[2]);
  enter(fc[2], fc[0]);
}

struct D3 {
  double x, y, z;
};
__device__ __forceinline__ double ddot(const D3 &a, const D3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 dcross(const D3 &a, const D3 &b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

__device__ __forceinline__ void add_q32(unsigned long long *sum, const D3 &u, double w) {
  atomicAdd(sum + 0, (unsigned long long)llrint((w * u.x) * Q32));
  atomicAdd(sum + 1, (unsigned long long)llrint((w * u.y) * Q32));
  atomicAdd(sum + 2, (unsigned long long)llrint((w * u.z) * Q32));
}

__global__ __launch_bounds__(256) void k_vox_normals(const float4 *__restrict__ records,
                                                    const int32_t *__restrict__ faces,
                                                    const uint8_t *__restrict__ usable, int ntri,
                                                    const uint64_t *__restrict__ ekeys, int64_t cap,
                                                    unsigned long long *vsum, unsigned long long *esum) {
  const int t = (int)(blockIdx.x * 256 + threadIdx.x);
  if (t >= ntri || !usable[t]) return;
  const float4 rb = records[(int64_t)t * 3 + 1], rc = records[(int64_t)t * 3 + 2];
  const D3 ab = {(double)rb.x, (double)rb.y, (double)rb.z}, ac = {(double)rc.x, (double)rc.y, (double)rc.z};
  const D3 n = dcross(ab, ac);
  const double len = sqrt(ddot(n, n));
  if (!(len > 0.0) || !isfinite(len)) return;                     // contributes nothing
  const D3 u = {n.x / len, n.y / len, n.z / len};
  const double g11 = ddot(ab, ab), g12 = ddot(ab, ac), g22 = ddot(ac, ac);
  const double angle[3] = {atan2(len, g12), atan2(len, g11 - g12), atan2(len, g22 - g12)};
  const int32_t *fc = faces + (int64_t)t * 3;
  const int v[3] = {fc[0], fc[1], fc[2]};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    add_q32(vsum + (int64_t)v[k] * 3, u, angle[k]);
    const uint64_t key = edge_key(v[k], v[(k + 1) % 3]);
    const int64_t slot = first_find<true>(ekeys, cap, edge_home(key, cap), [&](uint64_t q) { return q == key; });
    add_q32(esum + slot * 3, u, 1.0);
  }
}

struct Tables {
  const float4 *records;
  const int32_t *faces;
  const long long *vsum, *esum;
  const uint64_t *ekeys;
  int64_t cap;
};

// rules 4 and 6: s = dot(e, N) in fp64 with N the pseudo-normal of the feature of face f closest to p
__device__ __forceinline__ double vox_side(const V3 &p, int f, const Tables &tb) {
  const float4 ra = tb.records[(int64_t)f * 3], rb = tb.records[(int64_t)f * 3 + 1], rc = tb.records[(int64_t)f * 3 + 2];
  const V3 ab = {rb.x, rb.y, rb.z}, ac = {rc.x, rc.y, rc.z};
  int feature;
  const V3 e = tri_residual(p, {ra.x, ra.y, ra.z}, ab, ac, feature);
  D3 N;
  if (feature == TRI_INTERIOR) {
    N = dcross({(double)ab.x, (double)ab.y, (double)ab.z}, {(double)ac.x, (double)ac.y, (double)ac.z});
  } else {
    const int32_t *fc = tb.faces + (int64_t)f * 3;
    const long long *sum;
    if (feature <= TRI_VERT_C) {
      sum = tb.vsum + (int64_t)fc[feature] * 3;
    } else {
      const int i = fc[feature == TRI_EDGE_BC ? 1 : 0], j = fc[feature == TRI_EDGE_AB ? 1 : 2];
      const uint64_t key = edge_key(i, j);
      sum = tb.esum + 3 * first_find<true>(tb.ekeys, tb.cap, edge_home(key, tb.cap),
                                           [&](uint64_t q) { return q == key; });   // present: k_vox_edges ran first
    }
    N = {(double)sum[0] * (1.0 / Q32), (double)sum[1] * (1.0 / Q32), (double)sum[2] * (1.0 / Q32)};
  }
  return ddot({(double)e.x, (double)e.y, (double)e.z}, N);
}

__global__ __launch_bounds__(256) void k_vox_nearest(Tables tb, const float *__restrict__ boxes,
                                                    const int32_t *__restrict__ offsets,
                                                    const int32_t *__restrict__ refs,
                                                    const int32_t *__restrict__ bricks, int dx, int dy, int dz, float band,
                                                    int flip, float *__restrict__ dist, int32_t *__restrict__ face) {
  __shared__ float4 s_rec[BATCH * 3];
  __shared__ float s_box[BATCH * 6];
  __shared__ int s_id[BATCH];
  const int nbx = (dx + BRICK - 1) / BRICK, nby = (dy + BRICK - 1) / BRICK;
  const int brick = bricks[blockIdx.x], tid = (int)threadIdx.x;
  const int x = (brick % nbx) * BRICK + (tid & 7), y = ((brick / nbx) % nby) * BRICK + ((tid >> 3) & 7);
  const int z[2] = {(brick / (nbx * nby)) * BRICK + (tid >> 6), (brick / (nbx * nby)) * BRICK + (tid >> 6) + 4};
  const bool inside[2] = {x < dx && y < dy && z[0] < dz, x < dx && y < dy && z[1] < dz};
  const V3 p[2] = {{(float)x, (float)y, (float)z[0]}, {(float)x, (float)y, (float)z[1]}};
  const float inf = __int_as_float(0x7F800000), dmax = (float)max(dx, max(dy, dz));
  float best[2] = {inf, inf};
  int bt[2] = {-1, -1};
  const int beg = offsets[brick], end = offsets[brick + 1];
  for (int base = beg; base < end; base += BATCH) {
    const int n = min(BATCH, end - base);
    __syncthreads();                                              // the last batch has been read
    int f = 0;
    if (tid < n) s_id[tid] = f = refs[base + tid];                // the one read of the brick's list
    __syncthreads();
    if (tid < n) {
      float lo[3], hi[3];
      vox_box(boxes + (int64_t)f * 6, band, dmax, lo, hi);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        s_box[tid * 6 + k] = lo[k];
        s_box[tid * 6 + 3 + k] = hi[k];
      }
    }
    for (int q = tid; q < 3 * n; q += 256) {                      // three consecutive lanes read one 48-byte record
      const int slot = q / 3;
      s_rec[q] = tb.records[(int64_t)s_id[slot] * 3 + (q - 3 * slot)];
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {                                 // every lane reads the same LDS words: broadcasts
      const float *b = s_box + k * 6;
      const bool xy = p[0].x >= b[0] && p[0].x <= b[3] && p[0].y >= b[1] && p[0].y <= b[4];
      const bool in0 = inside[0] && xy && p[0].z >= b[2] && p[0].z <= b[5];
      const bool in1 = inside[1] && xy && p[1].z >= b[2] && p[1].z <= b[5];
      if (!(in0 || in1)) continue;
      const float4 ra = s_rec[k * 3], rb = s_rec[k * 3 + 1], rc = s_rec[k * 3 + 2];
      const V3 a = {ra.x, ra.y, ra.z}, ab = {rb.x, rb.y, rb.z}, ac = {rc.x, rc.y, rc.z};
      const int t = s_id[k];
#pragma unroll
      for (int v = 0; v < 2; ++v)
        if (v == 0 ? in0 : in1) {
          const float d2 = tri_dist2(p[v], a, ab, ac);
          if (d2 < best[v] || (d2 == best[v] && t < bt[v])) {
            best[v] = d2;
            bt[v] = t;
          }
        }
    }
  }
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    if (!inside[v]) continue;
    // correctly rounded: the fp64 root of an fp32 number, rounded once more, is the nearest fp32 (53 >= 2 * 24 + 2)
    float d = (float)sqrt((double)best[v]);
    int t = bt[v];
    if (!(d <= band) || t < 0) {
      d = inf;
      t = -1;
    } else {
      const double s = vox_side(p[v], t, tb);
      if (!((flip ? -s : s) >= 0.0)) d = -d;
    }
    const int64_t o = ((int64_t)z[v] * dy + y) * dx + x;
    dist[o] = d;
    face[o] = t;
  }
}

__global__ __launch_bounds__(256) void k_vox_tsdf(const float *__restrict__ dist, const int32_t *__restrict__ face,
                                                 int64_t n, float voxel_size, float *__restrict__ sdf,
                                                 uint8_t *__restrict__ weight) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool in = face[i] >= 0;
  sdf[i] = in ? dist[i] * voxel_size : -__int_as_float(0x7F800000);
  weight[i] = in ? 1 : 0;
}

bool dims_ok(int dx, int dy, int dz) {
  return dx >= 1 && dy >= 1 && dz >= 1 && dx <= 65535 && dy <= 65535 && dz <= 65535 &&
         (int64_t)dx * dy * dz < ((int64_t)1 << 31);
}

}  // namespace

SGNN_EXPORT int sgnn_vox_grid_coords(const float *verts, int64_t nv, const float *world2grid, float *out,
                                     sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nv >= 0 && nv < ((int64_t)1 << 31) && world2grid);
  if (nv == 0) return SGNN_OK;
  SGNN_CHECK_ARG(verts && out);
  TsdfAffine a;
  for (int k = 0; k < 12; ++k) a.m[k] = world2grid[k];
  SGNN_LAUNCH(k_vox_grid_coords, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts, nv, a, out);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_vox_bricks_count(const float *boxes, int ntri, float band, int dx, int dy, int dz, int32_t *counts,
                                      sgnn_stream_t stream) {
  SGNN_CHECK_ARG(ntri >= 0 && band >= 0.f && band <= 65535.f && dims_ok(dx, dy, dz));
  if (ntri == 0) return SGNN_OK;
  SGNN_CHECK_ARG(boxes && counts);
  SGNN_LAUNCH(k_vox_bricks<false>, dim3((ntri + 255) / 256), dim3(256), 0, (hipStream_t)stream, boxes, ntri, band, dx, dy,
              dz, (const int32_t *)nullptr, counts, (int32_t *)nullptr);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_vox_bricks_fill(const float *boxes, int ntri, float band, int dx, int dy, int dz,
                                     const int32_t *offsets, int32_t *cursor, int32_t *refs, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(ntri >= 0 && band >= 0.f && band <= 65535.f && dims_ok(dx, dy, dz));
  if (ntri == 0) return SGNN_OK;
  SGNN_CHECK_ARG(boxes && offsets && cursor && refs);
  SGNN_LAUNCH(k_vox_bricks<true>, dim3((ntri + 255) / 256), dim3(256), 0, (hipStream_t)stream, boxes, ntri, band, dx, dy,
              dz, offsets, cursor, refs);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_vox_normals(const float *records, const int32_t *faces, const uint8_t *usable, int ntri, int nverts,
                                 int64_t *vsum, int64_t *ekeys, int32_t *efirst, int64_t *esum, int64_t cap,
                                 sgnn_stream_t stream) {
  SGNN_CHECK_ARG(ntri >= 0 && nverts >= 0 && (int64_t)ntri * 3 < ((int64_t)1 << 31) &&
                 cap >= sgnn_weld_slots((int64_t)ntri * 3) && ekeys && efirst && esum && (nverts == 0 || vsum));
  const hipStream_t s = (hipStream_t)stream;
  void *const regions[2] = {vsum, esum};
  const int64_t words[2] = {(int64_t)nverts * 6, cap * 6};
  int rc = sgnn_fill32_multi(regions, words, 2, 0u, s);
  if (rc == SGNN_OK) rc = sgnn_fill32(ekeys, 0xFFFFFFFFu, 2 * cap, s);      // SLOT_EMPTY
  if (rc == SGNN_OK) rc = sgnn_fill32(efirst, 0x7F7F7F7Fu, cap, s);
  if (rc != SGNN_OK) return rc;
  if (ntri == 0) return SGNN_OK;
  SGNN_CHECK_ARG(records && faces && usable && ((uintptr_t)records & 15) == 0);
  const dim3 grid((ntri + 255) / 256);
  SGNN_LAUNCH(k_vox_edges, grid, dim3(256), 0, s, faces, usable, ntri, (uint64_t *)ekeys, efirst, cap);
  SGNN_LAUNCH(k_vox_normals, grid, dim3(256), 0, s, reinterpret_cast<const float4 *>(records), faces, usable, ntri,
              (const uint64_t *)ekeys, cap, (unsigned long long *)vsum, (unsigned long long *)esum);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_vox_nearest(const float *records, const float *boxes, const int32_t *faces, const int32_t *offsets,
                                 const int32_t *refs, const int32_t *bricks, int nbricks, int dx, int dy, int dz,
                                 float band, int flip, const int64_t *vsum, const int64_t *ekeys, const int64_t *esum,
                                 int64_t cap, float *dist, int32_t *face, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nbricks >= 0 && band >= 0.f && band <= 65535.f && dims_ok(dx, dy, dz) && cap >= 1);
  if (nbricks == 0) return SGNN_OK;
  SGNN_CHECK_ARG(records && boxes && faces && offsets && refs && bricks && vsum && ekeys && esum && dist && face);
  SGNN_CHECK_ARG(((uintptr_t)records & 15) == 0);
  SGNN_CHECK_ARG((int64_t)nbricks <= (int64_t)((dx + BRICK - 1) / BRICK) * ((dy + BRICK - 1) / BRICK) * ((dz + BRICK - 1) / BRICK));
  const Tables tb = {reinterpret_cast<const float4 *>(records), faces, (const long long *)vsum, (const long long *)esum,
                     (const uint64_t *)ekeys, cap};
  SGNN_LAUNCH(k_vox_nearest, dim3((unsigned)nbricks), dim3(256), 0, (hipStream_t)stream, tb, boxes, offsets, refs, bricks,
              dx, dy, dz, band, flip, dist, face);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_vox_tsdf(const float *dist, const int32_t *face, int64_t n, float voxel_size, float *sdf,
                              uint8_t *weight, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31));
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(dist && face && sdf && weight);
  SGNN_LAUNCH(k_vox_tsdf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dist, face, n, voxel_size,
              sdf, weight);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
