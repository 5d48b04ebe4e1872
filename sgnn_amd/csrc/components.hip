// Connected components of voxel masks and of index-sharing triangle meshes (include/sgnn_hip.h, "Connected
// components"; rules in INTEGRATION.md section J).  Integer work only.
//
// Union-find on parent[] (i32, one slot per voxel / vertex, -1 = background).  A hook always points the larger root at
// the smaller one with an atomic minimum, so parent[i] <= i at all times: every walk strictly decreases and ends, and
// the root of a finished component is its smallest index, which is what the numbering of the caller rests on.
//
// Memory model.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed by another CU's stores, so inside
// a merge kernel every access to a parent[] that another workgroup may write is an agent-scope atomic (relaxed loads
// for the walks, atomicMin for the hooks); there is no plain load of it.  A link that is out of date still points
// into the same component and the atomic returns the true old value, so the retry loop is correct whatever a walk
// saw.  Ordering between the passes comes from kernel boundaries only: no grid barrier, no flag that a workgroup
// waits on another for, and every loop makes progress on its own.
//
//   k_cc_tile     one workgroup per SGNN_CC_TILE tile: the same union-find in LDS (LDS atomics, two barriers), then
//                 the tile's forest goes to parent[] as global indices.  Raster order inside a tile is monotone in
//                 the global index, so parent[i] <= i holds for what it writes.
//   k_cc_border   one thread per voxel; ALL = false: unions the forward pairs that straddle a tile face, edge or
//                 corner; ALL = true (after k_cc_init): every forward pair, the one-level path.
//   k_cc_flatten  parent[i] = find(i), is_root[i]
//   k_cc_relabel  labels[i] = rank[parent[i]]; sizes with one 64-bit integer atomic per (wave, label)
//   k_cc_mesh_*   the same device functions on a parent[] of vertices, one thread per face
#include "common.h"

namespace {

constexpr int TZ = SGNN_CC_TILE_Z, TY = SGNN_CC_TILE_Y, TX = SGNN_CC_TILE_X;
constexpr int TILE = TZ * TY * TX;     // 2048 voxels: 8 KiB of LDS per workgroup, 8 voxels per thread
static_assert(TY * TX == 256, "a workgroup of 256 threads covers one z slice of a tile");

// the forward half of the 3 x 3 x 3 neighbourhood, (dz, dy, dx) > (0, 0, 0) in lexicographic order:
// 3 of the 6 faces, 6 of the 12 edges, 4 of the 8 corners
__device__ constexpr int8_t FWD[13][3] = {{0, 0, 1},  {0, 1, 0},  {1, 0, 0},                                   // faces
                                          {0, 1, -1}, {0, 1, 1},  {1, -1, 0}, {1, 1, 0},  {1, 0, -1}, {1, 0, 1},   // edges
                                          {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};                       // corners
__device__ __forceinline__ constexpr int fwd_class(int k) { return k < 3 ? 1 : k < 9 ? 2 : 3; }

__device__ __forceinline__ int32_t cc_load(const int32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x; x is foreground (parent[x] >= 0).  Every step goes to a smaller index.
__device__ __forceinline__ int32_t cc_find(const int32_t *parent, int32_t x) {
  int32_t p;
  while ((p = cc_load(parent + x)) != x && p >= 0) x = p;
  return x;
}

// joins the components of a and b (both foreground) and returns an index of the joined component that was a root
// when it was last seen: a good place to start the next walk from
__device__ __forceinline__ int32_t cc_union(int32_t *parent, int32_t a, int32_t b) {
  while (true) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return a;
    const int32_t hi = max(a, b), lo = min(a, b);
    const int32_t old = atomicMin(parent + hi, lo);
    if (old == hi) return lo;     // hi was still a root and now hangs below lo
    a = old;                      // hi had been hooked meanwhile: its former parent and lo remain to be joined
    b = lo;
  }
}

__global__ __launch_bounds__(256) void k_cc_tile(const uint8_t *__restrict__ mask, int dz, int dy, int dx, int tiles_z,
                                                 int tiles_y, int tiles_x, int maxc, int32_t *__restrict__ parent) {
  __shared__ int32_t lab[TILE];
  unsigned t = blockIdx.x;
  const int bx = (int)(t % (unsigned)tiles_x);
  t /= (unsigned)tiles_x;
  const int by = (int)(t % (unsigned)tiles_y);
  t /= (unsigned)tiles_y;
  const int bz = (int)(t % (unsigned)tiles_z);
  const int b = (int)(t / (unsigned)tiles_z);
  const int tid = (int)threadIdx.x, lx = tid % TX, ly = tid / TX;
  const int z0 = bz * TZ, y = by * TY + ly, x = bx * TX + lx;
  const bool in_yx = y < dy && x < dx;
  // global index of local voxel (k, ly, lx) of this thread's column: col + k * dy * dx
  const int64_t slice = (int64_t)dy * dx;
  const int64_t col = (((int64_t)b * dz + z0) * dy + y) * dx + x;
  unsigned fg = 0;
#pragma unroll
  for (int k = 0; k < TZ; ++k) {
    const bool f = in_yx && z0 + k < dz && mask[col + k * slice] != 0;
    fg |= (unsigned)f << k;
    lab[k * 256 + tid] = f ? k * 256 + tid : -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TZ; ++k) {
    if (!((fg >> k) & 1u)) continue;
    int32_t root = k * 256 + tid;
#pragma unroll
    for (int o = 0; o < 13; ++o) {
      if (fwd_class(o) > maxc) continue;
      const int nz = k + FWD[o][0], ny = ly + FWD[o][1], nx = lx + FWD[o][2];
      if (nz >= TZ || (unsigned)ny >= (unsigned)TY || (unsigned)nx >= (unsigned)TX) continue;
      const int32_t m = (nz * TY + ny) * TX + nx;
      if (cc_load(lab + m) >= 0) root = cc_union(lab, root, m);      // a voxel outside the volume holds -1
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TZ; ++k) {
    if (!(in_yx && z0 + k < dz)) continue;
    int32_t out = -1;
    if ((fg >> k) & 1u) {
      const int32_t r = cc_find(lab, k * 256 + tid);
      const int rz = r / 256, ry = (r / TX) % TY, rx = r % TX;
      out = (int32_t)((((int64_t)b * dz + z0 + rz) * dy + by * TY + ry) * dx + bx * TX + rx);
    }
    parent[col + k * slice] = out;
  }
}

__global__ __launch_bounds__(256) void k_cc_init(const uint8_t *__restrict__ mask, int64_t n,
                                                 int32_t *__restrict__ parent) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) parent[i] = mask[i] ? (int32_t)i : -1;
}

template <bool ALL>
__global__ __launch_bounds__(256) void k_cc_border(const uint8_t *__restrict__ mask, int64_t n, int dz, int dy, int dx,
                                                   int maxc, int32_t *parent) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int x = (int)(v % dx);
  const int64_t r1 = v / dx;
  const int y = (int)(r1 % dy), z = (int)((r1 / dy) % dz);
  const int lz = z % TZ, ly = y % TY, lx = x % TX;
  if (!ALL && lz < TZ - 1 && ly > 0 && ly < TY - 1 && lx > 0 && lx < TX - 1) return;   // no forward pair leaves the tile
  if (!mask[v]) return;
  int32_t root = (int32_t)v;
#pragma unroll
  for (int o = 0; o < 13; ++o) {
    if (fwd_class(o) > maxc) continue;
    const int oz = FWD[o][0], oy = FWD[o][1], ox = FWD[o][2];
    const int nz = z + oz, ny = y + oy, nx = x + ox;
    if (nz >= dz || (unsigned)ny >= (unsigned)dy || (unsigned)nx >= (unsigned)dx) continue;   // inside this sample only
    if (!ALL && lz + oz < TZ && (unsigned)(ly + oy) < (unsigned)TY && (unsigned)(lx + ox) < (unsigned)TX) continue;
    const int64_t m = v + ((int64_t)oz * dy + oy) * dx + ox;
    if (mask[m]) root = cc_union(parent, root, (int32_t)m);
  }
  if (root < (int32_t)v) atomicMin(parent + v, root);     // root is an ancestor of v: a shorter walk for the next pass
}

__global__ __launch_bounds__(256) void k_cc_flatten(int32_t *parent, int64_t n, uint8_t *__restrict__ is_root) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t p = cc_load(parent + i);
  if (p < 0) {
    is_root[i] = 0;
    return;
  }
  // other threads of this launch replace links by roots meanwhile: either is a link into the same tree
  const int32_t r = cc_find(parent, p);
  if (r != p) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  is_root[i] = r == (int32_t)i;
}

// sizes[label] += 1 for every lane with a label in [0, ncomp): one atomic per distinct label of the wave
__device__ __forceinline__ void cc_count(int32_t label, int64_t ncomp, int64_t *sizes) {
  const bool valid = label >= 0 && (int64_t)label < ncomp;
  const int lane = (int)(threadIdx.x & 63);
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int32_t l = __shfl(label, leader);
    const unsigned long long same = __ballot(valid && label == l);
    if (lane == leader) atomicAdd(reinterpret_cast<unsigned long long *>(sizes) + l, (unsigned long long)__popcll(same));
    todo &= ~same;
  }
}

__global__ __launch_bounds__(256) void k_cc_relabel(const int32_t *__restrict__ parent, int64_t n,
                                                    const int32_t *__restrict__ rank, int64_t ncomp,
                                                    int32_t *__restrict__ labels, int64_t *sizes) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int32_t label = -1;
  if (i < n) {
    const int32_t p = parent[i];
    if (p >= 0 && (int64_t)p < n) label = rank[p];
    labels[i] = label;
  }
  cc_count(label, ncomp, sizes);
}

__global__ __launch_bounds__(256) void k_cc_mesh_mark(const int32_t *__restrict__ faces, int ntri, int nverts,
                                                      int32_t *parent, int32_t *status) {
  const int t = (int)(blockIdx.x * 256 + threadIdx.x);
  bool bad = false;
  if (t < ntri) {
    const int32_t *fc = faces + (int64_t)t * 3;
    const int i0 = fc[0], i1 = fc[1], i2 = fc[2];
    bad = (uint32_t)i0 >= (uint32_t)nverts || (uint32_t)i1 >= (uint32_t)nverts || (uint32_t)i2 >= (uint32_t)nverts;
    if (!bad) {      // every writer of a slot stores the same value
      __hip_atomic_store(parent + i0, i0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(parent + i1, i1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(parent + i2, i2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (status && __ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(status, SGNN_STATUS_COORD_RANGE);
}

__global__ __launch_bounds__(256) void k_cc_mesh_link(const int32_t *__restrict__ faces, int ntri, int nverts,
                                                      int32_t *parent) {
  const int t = (int)(blockIdx.x * 256 + threadIdx.x);
  if (t >= ntri) return;
  const int32_t *fc = faces + (int64_t)t * 3;
  const int i0 = fc[0], i1 = fc[1], i2 = fc[2];
  if ((uint32_t)i0 >= (uint32_t)nverts || (uint32_t)i1 >= (uint32_t)nverts || (uint32_t)i2 >= (uint32_t)nverts) return;
  const int32_t root = cc_union(parent, i0, i1);
  cc_union(parent, root, i2);
}

__global__ __launch_bounds__(256) void k_cc_face_labels(const int32_t *__restrict__ faces, int ntri, int nverts,
                                                        const int32_t *__restrict__ vertex_labels, int64_t ncomp,
                                                        int32_t *__restrict__ face_labels, int64_t *face_sizes) {
  const int t = (int)(blockIdx.x * 256 + threadIdx.x);
  int32_t label = -1;
  if (t < ntri) {
    const int32_t *fc = faces + (int64_t)t * 3;
    const int i0 = fc[0], i1 = fc[1], i2 = fc[2];
    if ((uint32_t)i0 < (uint32_t)nverts && (uint32_t)i1 < (uint32_t)nverts && (uint32_t)i2 < (uint32_t)nverts)
      label = vertex_labels[i0];
    face_labels[t] = label;
  }
  cc_count(label, ncomp, face_sizes);
}

constexpr int64_t LIMIT = (int64_t)1 << 31;

}  // namespace

SGNN_EXPORT int sgnn_cc_volume_link(const uint8_t *mask, int nb, int dz, int dy, int dx, int connectivity, int tiled,
                                    int32_t *parent, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nb >= 0 && dz >= 0 && dy >= 0 && dx >= 0);
  SGNN_CHECK_ARG(connectivity == 6 || connectivity == 18 || connectivity == 26);
  const int64_t plane = (int64_t)dy * dx;
  SGNN_CHECK_ARG(plane < LIMIT && (int64_t)nb * dz < LIMIT);
  const int64_t n = (int64_t)nb * dz * plane;
  SGNN_CHECK_ARG(n < LIMIT);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(mask && parent);
  const int maxc = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 per_voxel((unsigned)((n + 255) / 256));
  if (tiled) {
    const int tz = (dz + TZ - 1) / TZ, ty = (dy + TY - 1) / TY, tx = (dx + TX - 1) / TX;
    const int64_t tiles = (int64_t)nb * tz * ty * tx;       // <= n < 2^31
    SGNN_LAUNCH(k_cc_tile, dim3((unsigned)tiles), dim3(256), 0, s, mask, dz, dy, dx, tz, ty, tx, maxc, parent);
    SGNN_CHECK_LAUNCH();
    SGNN_LAUNCH(k_cc_border<false>, per_voxel, dim3(256), 0, s, mask, n, dz, dy, dx, maxc, parent);
  } else {
    SGNN_LAUNCH(k_cc_init, per_voxel, dim3(256), 0, s, mask, n, parent);
    SGNN_CHECK_LAUNCH();
    SGNN_LAUNCH(k_cc_border<true>, per_voxel, dim3(256), 0, s, mask, n, dz, dy, dx, maxc, parent);
  }
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_cc_mesh_link(const int32_t *faces, int ntri, int nverts, int32_t *parent, int32_t *status,
                                  sgnn_stream_t stream) {
  SGNN_CHECK_ARG(ntri >= 0 && nverts >= 0 && (int64_t)ntri * 3 < LIMIT);
  if (nverts == 0 && ntri == 0) return SGNN_OK;
  SGNN_CHECK_ARG((nverts == 0 || parent) && (ntri == 0 || faces));
  const hipStream_t s = (hipStream_t)stream;
  if (nverts) {
    const int rc = sgnn_fill32(parent, 0xFFFFFFFFu, nverts, s);      // -1: not referenced by any face
    if (rc != SGNN_OK) return rc;
  }
  if (ntri == 0) return SGNN_OK;
  const dim3 per_face((unsigned)((ntri + 255) / 256));
  SGNN_LAUNCH(k_cc_mesh_mark, per_face, dim3(256), 0, s, faces, ntri, nverts, parent, status);
  SGNN_CHECK_LAUNCH();
  SGNN_LAUNCH(k_cc_mesh_link, per_face, dim3(256), 0, s, faces, ntri, nverts, parent);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_cc_flatten(int32_t *parent, int64_t n, uint8_t *is_root, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && n < LIMIT);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(parent && is_root);
  SGNN_LAUNCH(k_cc_flatten, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, parent, n, is_root);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_cc_relabel(const int32_t *parent, int64_t n, const int32_t *rank, int64_t ncomp, int32_t *labels,
                                int64_t *sizes, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && n < LIMIT && ncomp >= 0 && ncomp <= n);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(parent && rank && labels && (ncomp == 0 || sizes));
  SGNN_LAUNCH(k_cc_relabel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, parent, n, rank, ncomp,
              labels, sizes);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_cc_face_labels(const int32_t *faces, int ntri, int nverts, const int32_t *vertex_labels,
                                    int64_t ncomp, int32_t *face_labels, int64_t *face_sizes, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(ntri >= 0 && nverts >= 0 && (int64_t)ntri * 3 < LIMIT && ncomp >= 0);
  if (ntri == 0) return SGNN_OK;
  SGNN_CHECK_ARG(faces && face_labels && (nverts == 0 || vertex_labels) && (ncomp == 0 || face_sizes));
  SGNN_LAUNCH(k_cc_face_labels, dim3((unsigned)((ntri + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, ntri,
              nverts, vertex_labels, ncomp, face_labels, face_sizes);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
