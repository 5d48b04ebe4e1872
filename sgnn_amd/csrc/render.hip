// Depth frames rendered from a triangle mesh (sgnn_amd.render): the "virtual scan" source of datagen/GenerateScans
// (Scene::renderDepthFrame), whose Direct3D rasteriser is not part of this project.  The rules are listed in
// INTEGRATION.md section F; that text is the contract, and tests/render_ref.py restates it independently in NumPy.
// Colour frames from a mesh with vertex colours are drawn by the same kernel text (template parameter COLOR); their
// rules are listed in section N and restated in tests/render_color_ref.py.
//
// Kernels:
//   k_render_clear      the output doubles as the depth buffer: +inf bit pattern, 16-byte stores
//   k_render_check      face indices outside [0, V) raise SGNN_STATUS_COORD_RANGE in the status word
//   k_render_triangles  grid = (triangle blocks, groups of FRAMES_PER_BLOCK frames).  A thread holds one triangle
//                       (face and three vertices loaded once) and walks the frames of its group; the frame record
//                       is workgroup-uniform and arrives by scalar loads.  Per (frame, triangle): transform, reject,
//                       near-plane clip, snap to 1/256 pixel, int64 edge functions, one 32-bit unsigned atomic
//                       minimum per covered pixel.  A triangle whose pixel box is large is rasterised by its whole
//                       wave, 64 consecutive box pixels per step.
//   k_render_finish     range test -> -inf, four pixels per thread
// With COLOR the depth buffer is a workspace of 64-bit keys, z bits in the high word and R<<24 | G<<16 | B<<8 | 255 in
// the low word, folded with one 64-bit unsigned atomic minimum per covered pixel; k_rendercol_finish splits a key
// into the depth pixel and the R, G, B, A bytes.
//
// Built with -ffp-contract=off (Makefile): every product and sum is rounded on its own, and depth > 0 always, so the
// unsigned minimum of the bit patterns is the nearest depth whatever the order of triangles, frames and launches.
#include <math.h>
#include <type_traits>
#include "common.h"
#include "geom.h"   // the affine row of transform() and the pinhole of snap()

namespace {

constexpr int FRAMES_PER_BLOCK = 8;        // frames a thread walks with its triangle in registers
constexpr int WAVE_PIXELS_DEFAULT = 128;   // pixel boxes above this are rasterised by the whole wave
constexpr uint32_t INF_BITS = 0x7F800000u;
constexpr float SNAP_LIMIT = 536870912.0f;   // 2^29: keeps every edge function inside int64

struct Vec3 {
  float x, y, z;
};

// the colour a vertex carries, three fp32 channels in 0..255; nothing in the depth-only kernel
template <bool COLOR>
struct Col {};
template <>
struct Col<true> {
  float c[3];
};

template <bool COLOR>
using Pix = typename std::conditional<COLOR, uint64_t, uint32_t>::type;   // one pixel of the depth buffer

// one screen triangle ready for rasterisation: e_k(i, j) = c_k + dx_k * (i - i0) + dy_k * (j - j0) at pixel (i, j)
template <bool COLOR>
struct Setup {
  int64_t c[3];
  int64_t dx[3], dy[3];   // steps per pixel: -256 (yb - ya), 256 (xb - xa)
  float r[3];             // 1 / z_k
  float area;             // (float)A2
  int i0, j0, bw, bh;     // pixel box clamped to the image; bw == 0: nothing to draw
  Col<COLOR> col[3];      // the colour of vertex k
};

__device__ __forceinline__ Vec3 transform(const float *m, float x, float y, float z) {
  return Vec3{tsdf_affine_row(m, 0, x, y, z), tsdf_affine_row(m, 1, x, y, z), tsdf_affine_row(m, 2, x, y, z)};
}

// the point where edge a -> b meets z = zc, always from the kept end a towards the dropped end b
__device__ __forceinline__ Vec3 clip_point(const Vec3 &a, const Vec3 &b, float zc) {
  const float t = __fdiv_rn(zc - a.z, b.z - a.z);
  Vec3 c;
  c.x = a.x + t * (b.x - a.x);
  c.y = a.y + t * (b.y - a.y);
  c.z = zc;
  return c;
}

// the colour at that point: the same t, from the kept end towards the dropped end
__device__ __forceinline__ Col<false> clip_color(const Vec3 &, const Vec3 &, float, const Col<false> &,
                                                 const Col<false> &) {
  return Col<false>();
}
__device__ __forceinline__ Col<true> clip_color(const Vec3 &a, const Vec3 &b, float zc, const Col<true> &ca,
                                                const Col<true> &cb) {
  const float t = __fdiv_rn(zc - a.z, b.z - a.z);
  Col<true> c;
#pragma unroll
  for (int k = 0; k < 3; ++k) c.c[k] = ca.c[k] + t * (cb.c[k] - ca.c[k]);
  return c;
}

// rule 4: project and snap to 1/256 pixel; false when the vertex cannot be snapped
__device__ __forceinline__ bool snap(const Vec3 &p, const float *intr, int64_t &X, int64_t &Y) {
  const float u = geom_project(intr, 0, p.x, p.z), v = geom_project(intr, 1, p.y, p.z);
  const float sx = roundf(u * 256.0f), sy = roundf(v * 256.0f);   // half away from zero
  if (!(fabsf(sx) <= SNAP_LIMIT && fabsf(sy) <= SNAP_LIMIT)) return false;   // NaN and inf fail
  X = (int64_t)sx;
  Y = (int64_t)sy;
  return true;
}

__device__ __forceinline__ int64_t edge(int64_t xa, int64_t ya, int64_t xb, int64_t yb, int64_t px, int64_t py) {
  return (xb - xa) * (py - ya) - (yb - ya) * (px - xa);
}

// rules 4-6 for one camera-space triangle with all z >= z_clip
template <bool COLOR>
__device__ __forceinline__ void setup_triangle(const Vec3 &a, const Vec3 &b, const Vec3 &c, const Col<COLOR> &ca,
                                               const Col<COLOR> &cb, const Col<COLOR> &cc, const float *intr, int h,
                                               int w, Setup<COLOR> &s) {
  s.bw = 0;
  int64_t X[3], Y[3];
  if (!(snap(a, intr, X[0], Y[0]) && snap(b, intr, X[1], Y[1]) && snap(c, intr, X[2], Y[2]))) return;
  float z1 = b.z, z2 = c.z;
  s.col[0] = ca;
  s.col[1] = cb;
  s.col[2] = cc;
  int64_t a2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0]);
  if (a2 == 0) return;
  if (a2 < 0) {                      // no culling: turn the triangle over
    a2 = -a2;
    int64_t t = X[1]; X[1] = X[2]; X[2] = t;
    t = Y[1]; Y[1] = Y[2]; Y[2] = t;
    const float tz = z1; z1 = z2; z2 = tz;
    s.col[1] = cc;
    s.col[2] = cb;
  }
  const int64_t xmin = min(X[0], min(X[1], X[2])), xmax = max(X[0], max(X[1], X[2]));
  const int64_t ymin = min(Y[0], min(Y[1], Y[2])), ymax = max(Y[0], max(Y[1], Y[2]));
  const int64_t i0 = max((xmin + 255) >> 8, (int64_t)0), i1 = min(xmax >> 8, (int64_t)w - 1);
  const int64_t j0 = max((ymin + 255) >> 8, (int64_t)0), j1 = min(ymax >> 8, (int64_t)h - 1);
  if (i0 > i1 || j0 > j1) return;
  const int64_t px = i0 * 256, py = j0 * 256;
  s.c[0] = edge(X[1], Y[1], X[2], Y[2], px, py);     // e_k is opposite vertex k; e0 + e1 + e2 = A2
  s.c[1] = edge(X[2], Y[2], X[0], Y[0], px, py);
  s.c[2] = edge(X[0], Y[0], X[1], Y[1], px, py);
  s.dx[0] = -256 * (Y[2] - Y[1]); s.dy[0] = 256 * (X[2] - X[1]);
  s.dx[1] = -256 * (Y[0] - Y[2]); s.dy[1] = 256 * (X[0] - X[2]);
  s.dx[2] = -256 * (Y[1] - Y[0]); s.dy[2] = 256 * (X[1] - X[0]);
  s.r[0] = __fdiv_rn(1.0f, a.z);
  s.r[1] = __fdiv_rn(1.0f, z1);
  s.r[2] = __fdiv_rn(1.0f, z2);
  s.area = (float)a2;
  s.i0 = (int)i0;
  s.j0 = (int)j0;
  s.bw = (int)(i1 - i0) + 1;
  s.bh = (int)(j1 - j0) + 1;
}

// one channel of a pixel: roundf, half away from zero, clamped to 0..255 (a NaN gives 0)
__device__ __forceinline__ uint32_t channel8(float c) {
  const float v = roundf(c);
  return v >= 255.0f ? 255u : (v >= 0.0f ? (uint32_t)v : 0u);
}

// rule 7 and the depth test of rule 8; with COLOR the pixel colour and the key of section N
template <bool COLOR>
__device__ __forceinline__ void shade(Pix<COLOR> *pix, int64_t e0, int64_t e1, int64_t e2, const float *r, float area,
                                      const Col<COLOR> *col) {
  const float w0 = (float)e0 * r[0], w1 = (float)e1 * r[1], w2 = (float)e2 * r[2];
  const float q = (w0 + w1) + w2;
  const float z = __fdiv_rn(area, q);
  if constexpr (!COLOR) {
    __hip_atomic_fetch_min(pix, __float_as_uint(z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    // No look at the key's z word before this: skipping fragments that lie behind what such a load returns measured
    // 1.3 times slower on the bench scene (overdraw 1.6: few fragments lose, every one waits for the load).
    uint32_t rgb = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float c = __fdiv_rn((w0 * col[0].c[k] + w1 * col[1].c[k]) + w2 * col[2].c[k], q);
      rgb = (rgb << 8) | channel8(c);
    }
    const uint64_t key = ((uint64_t)__float_as_uint(z) << 32) | (uint64_t)((rgb << 8) | 255u);
    __hip_atomic_fetch_min(pix, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__device__ __forceinline__ int64_t readlane64(int64_t v, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), lane);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ float readlanef(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// Draw one set-up triangle per lane (s.bw == 0: none).  Small boxes are walked by their own lane; a box above
// wave_pixels is handed to the whole wave.  Every lane of the wave must call this (it ballots).
template <bool COUNT, bool COLOR>
__device__ __forceinline__ void draw(const Setup<COLOR> &s, Pix<COLOR> *__restrict__ frame, int w, int wave_pixels,
                                     unsigned long long *__restrict__ counters) {
  const bool any = s.bw > 0;
  const bool big = any && s.bw * s.bh > wave_pixels;
  unsigned long long npix = 0;
  if (any && !big) {
    int64_t r0 = s.c[0], r1 = s.c[1], r2 = s.c[2];
    for (int j = 0; j < s.bh; ++j) {
      int64_t e0 = r0, e1 = r1, e2 = r2;
      Pix<COLOR> *row = frame + (int64_t)(s.j0 + j) * w + s.i0;
      for (int i = 0; i < s.bw; ++i) {
        if ((e0 | e1 | e2) >= 0) {
          shade<COLOR>(row + i, e0, e1, e2, s.r, s.area, s.col);
          if (COUNT) ++npix;
        }
        e0 += s.dx[0];
        e1 += s.dx[1];
        e2 += s.dx[2];
      }
      r0 += s.dy[0];
      r1 += s.dy[1];
      r2 += s.dy[2];
    }
  }
  unsigned long long todo = __ballot(big);
  const int lane = (int)(threadIdx.x & 63);
  while (todo) {
    const int src = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(todo));
    todo &= todo - 1;
    int64_t c[3], dx[3], dy[3];
    float r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      c[k] = readlane64(s.c[k], src);
      dx[k] = readlane64(s.dx[k], src);
      dy[k] = readlane64(s.dy[k], src);
      r[k] = readlanef(s.r[k], src);
    }
    const float area = readlanef(s.area, src);
    Col<COLOR> col[3];
    if constexpr (COLOR) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) col[k].c[ch] = readlanef(s.col[k].c[ch], src);
    }
    const int i0 = __builtin_amdgcn_readlane(s.i0, src), j0 = __builtin_amdgcn_readlane(s.j0, src);
    const int bw = __builtin_amdgcn_readlane(s.bw, src), bh = __builtin_amdgcn_readlane(s.bh, src);
    const int total = bw * bh;
    for (int base = 0; base < total; base += 64) {
      const int idx = base + lane;
      if (idx < total) {
        const int row = idx / bw, column = idx - row * bw;
        const int64_t e0 = c[0] + dx[0] * column + dy[0] * row;
        const int64_t e1 = c[1] + dx[1] * column + dy[1] * row;
        const int64_t e2 = c[2] + dx[2] * column + dy[2] * row;
        if ((e0 | e1 | e2) >= 0) {
          shade<COLOR>(frame + (int64_t)(j0 + row) * w + (i0 + column), e0, e1, e2, r, area, col);
          if (COUNT) ++npix;
        }
      }
    }
  }
  if (COUNT) {
    if (any && !big) atomicAdd(counters + 0, 1ull);
    if (big) atomicAdd(counters + 1, 1ull);
    if (npix) atomicAdd(counters + 2, npix);
  }
}

template <uint32_t WORD>
__global__ __launch_bounds__(256) void k_render_clear(uint32_t *__restrict__ out, int64_t n) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint4 *o4 = reinterpret_cast<uint4 *>(out);
  for (int64_t q = t; q < n4; q += stride) o4[q] = make_uint4(WORD, WORD, WORD, WORD);
  if (t < (n & 3)) out[(n4 << 2) + t] = WORD;
}

__global__ __launch_bounds__(256) void k_render_check(const int32_t *__restrict__ faces, int64_t n, int nverts,
                                                     int32_t *__restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  bool bad = false;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += stride)
    bad = bad || (uint32_t)faces[q] >= (uint32_t)nverts;
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(status, SGNN_STATUS_COORD_RANGE);
}

template <bool COUNT, bool COLOR>
__global__ __launch_bounds__(256) void k_render_triangles(const float *__restrict__ verts, int nverts,
                                                         const int32_t *__restrict__ faces, int ntri,
                                                         const sgnn_render_frame *__restrict__ frames, int f0, int f1,
                                                         int h, int w, float zc, int wave_pixels,
                                                         Pix<COLOR> *__restrict__ out,
                                                         unsigned long long *__restrict__ counters,
                                                         const uint8_t *__restrict__ vcolors) {
  const int t = (int)(blockIdx.x * 256 + threadIdx.x);
  int ia = 0, ib = 0, ic = 0;
  bool have = t < ntri;
  if (have) {
    const int32_t *fc = faces + (int64_t)t * 3;
    const int i0 = fc[0], i1 = fc[1], i2 = fc[2];
    have = (uint32_t)i0 < (uint32_t)nverts && (uint32_t)i1 < (uint32_t)nverts && (uint32_t)i2 < (uint32_t)nverts;
    // smallest index first, cyclic order kept: the image then depends on a face's vertices, not on how it lists them
    if (i0 <= i1 && i0 <= i2) { ia = i0; ib = i1; ic = i2; }
    else if (i1 <= i2) { ia = i1; ib = i2; ic = i0; }
    else { ia = i2; ib = i0; ic = i1; }
  }
  float va[3] = {0.f, 0.f, 0.f}, vb[3] = {0.f, 0.f, 0.f}, vc[3] = {0.f, 0.f, 0.f};
  if (have) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      va[k] = verts[(int64_t)ia * 3 + k];
      vb[k] = verts[(int64_t)ib * 3 + k];
      vc[k] = verts[(int64_t)ic * 3 + k];
    }
  }
  Col<COLOR> c0, c1, c2;                            // carried with their vertices through the rotation above
  if constexpr (COLOR) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      c0.c[k] = have ? (float)vcolors[(int64_t)ia * 3 + k] : 0.f;
      c1.c[k] = have ? (float)vcolors[(int64_t)ib * 3 + k] : 0.f;
      c2.c[k] = have ? (float)vcolors[(int64_t)ic * 3 + k] : 0.f;
    }
  }
  const int fbeg = f0 + (int)blockIdx.y * FRAMES_PER_BLOCK;
  const int fend = min(fbeg + FRAMES_PER_BLOCK, f1);
  const int64_t frame_px = (int64_t)h * w;
  for (int f = fbeg; f < fend; ++f) {
    const sgnn_render_frame &F = frames[f];
    if (!(F.m[0] == F.m[0])) continue;            // non-finite pose (the host stores NaN): the frame stays empty
    Pix<COLOR> *frame = out + (int64_t)f * frame_px;
    const float *intr = F.intr;
    const Vec3 p0 = transform(F.m, va[0], va[1], va[2]);
    const Vec3 p1 = transform(F.m, vb[0], vb[1], vb[2]);
    const Vec3 p2 = transform(F.m, vc[0], vc[1], vc[2]);
    const bool k0 = p0.z >= zc, k1 = p1.z >= zc, k2 = p2.z >= zc;     // NaN: not kept
    const int nk = (int)k0 + (int)k1 + (int)k2;
    bool live = have && nk > 0;
    if (live) {
      // A half-space that holds all three vertices holds the triangle, and a point of it with z > 0 projects two
      // pixels or more outside the image: nothing can be covered.  (Two pixels is far above the rounding of these
      // products; a NaN fails every comparison and rejects nothing.)
      const float fx = intr[0], fy = intr[1];
      const float lx = -2.0f - intr[2], hx = (float)w + 1.0f - intr[2];
      const float ly = -2.0f - intr[3], hy = (float)h + 1.0f - intr[3];
      const bool left = p0.x * fx < lx * p0.z && p1.x * fx < lx * p1.z && p2.x * fx < lx * p2.z;
      const bool right = p0.x * fx > hx * p0.z && p1.x * fx > hx * p1.z && p2.x * fx > hx * p2.z;
      const bool above = p0.y * fy < ly * p0.z && p1.y * fy < ly * p1.z && p2.y * fy < ly * p2.z;
      const bool below = p0.y * fy > hy * p0.z && p1.y * fy > hy * p1.z && p2.y * fy > hy * p2.z;
      live = !(left || right || above || below);
    }
    // rule 3: up to two triangles (a, b, c) and (a, c, d)
    Vec3 a = p0, b = p1, c = p2, d = p2;
    Col<COLOR> ca = c0, cb = c1, cc = c2, cd = c2;
    int ntris = live ? 1 : 0;
    if (live && nk == 1) {
      const Vec3 ka = k0 ? p0 : (k1 ? p1 : p2);                        // the kept vertex, then its two successors
      const Vec3 n1 = k0 ? p1 : (k1 ? p2 : p0);
      const Vec3 n2 = k0 ? p2 : (k1 ? p0 : p1);
      a = ka;
      b = clip_point(ka, n1, zc);
      c = clip_point(ka, n2, zc);
      const Col<COLOR> cka = k0 ? c0 : (k1 ? c1 : c2);
      const Col<COLOR> cn1 = k0 ? c1 : (k1 ? c2 : c0);
      const Col<COLOR> cn2 = k0 ? c2 : (k1 ? c0 : c1);
      ca = cka;
      cb = clip_color(ka, n1, zc, cka, cn1);
      cc = clip_color(ka, n2, zc, cka, cn2);
    } else if (live && nk == 2) {
      const Vec3 dr = !k0 ? p0 : (!k1 ? p1 : p2);                      // the dropped vertex, then its two successors
      const Vec3 s1 = !k0 ? p1 : (!k1 ? p2 : p0);
      const Vec3 s2 = !k0 ? p2 : (!k1 ? p0 : p1);
      const int x1 = !k0 ? ib : (!k1 ? ic : ia), x2 = !k0 ? ic : (!k1 ? ia : ib);
      const bool sw = x2 < x1;                                          // apex: the kept vertex of smaller index
      const Vec3 ap = sw ? s2 : s1, ot = sw ? s1 : s2;
      a = ap;
      b = ot;
      c = clip_point(ot, dr, zc);
      d = clip_point(ap, dr, zc);
      const Col<COLOR> cdr = !k0 ? c0 : (!k1 ? c1 : c2);
      const Col<COLOR> cs1 = !k0 ? c1 : (!k1 ? c2 : c0);
      const Col<COLOR> cs2 = !k0 ? c2 : (!k1 ? c0 : c1);
      const Col<COLOR> cap = sw ? cs2 : cs1, cot = sw ? cs1 : cs2;
      ca = cap;
      cb = cot;
      cc = clip_color(ot, dr, zc, cot, cdr);
      cd = clip_color(ap, dr, zc, cap, cdr);
      ntris = 2;
    }
    Setup<COLOR> s = {};
    if (ntris >= 1) setup_triangle<COLOR>(a, b, c, ca, cb, cc, intr, h, w, s);
    draw<COUNT, COLOR>(s, frame, w, wave_pixels, counters);
    if (__ballot(ntris == 2)) {
      s.bw = 0;
      if (ntris == 2) setup_triangle<COLOR>(a, c, d, ca, cc, cd, intr, h, w, s);
      draw<COUNT, COLOR>(s, frame, w, wave_pixels, counters);
    }
  }
}

__global__ __launch_bounds__(256) void k_render_finish(uint32_t *__restrict__ out, int64_t n, float dmin, float dmax) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t ninf = 0xFF800000u;
  auto fin = [=](uint32_t v) {
    const float z = __uint_as_float(v);
    return (v != INF_BITS && z >= dmin && z <= dmax) ? v : ninf;
  };
  uint4 *o4 = reinterpret_cast<uint4 *>(out);
  for (int64_t q = t; q < n4; q += stride) {
    uint4 v = o4[q];
    v.x = fin(v.x);
    v.y = fin(v.y);
    v.z = fin(v.z);
    v.w = fin(v.w);
    o4[q] = v;
  }
  if (t < (n & 3)) out[(n4 << 2) + t] = fin(out[(n4 << 2) + t]);
}

// key -> depth pixel and R, G, B, A bytes; the range test of k_render_finish
__global__ __launch_bounds__(256) void k_rendercol_finish(const uint64_t *__restrict__ keys, int64_t n, float dmin,
                                                         float dmax, uint32_t *__restrict__ depth,
                                                         uint32_t *__restrict__ rgba) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += stride) {
    const uint64_t key = keys[q];
    const uint32_t zb = (uint32_t)(key >> 32);
    const float z = __uint_as_float(zb);
    const bool seen = key != ~0ull && zb != INF_BITS && z >= dmin && z <= dmax;
    depth[q] = seen ? zb : 0xFF800000u;
    rgba[q] = seen ? __builtin_bswap32((uint32_t)key) : 0u;      // memory order R, G, B, A
  }
}

// the launches of both entry points; COLOR: the depth buffer is `keys`, out and rgba are written by the finish
template <bool COLOR>
int render(const float *verts, int nverts, const int32_t *faces, int ntri, const sgnn_render_frame *frames, int nframes,
           int chunk, int h, int w, float z_clip, float depth_min, float depth_max, int wave_pixels, float *out,
           int32_t *status, int64_t *counters, const uint8_t *vcolors, uint64_t *keys, uint8_t *rgba,
           sgnn_stream_t stream) {
  SGNN_CHECK_ARG(nverts >= 0 && ntri >= 0 && nframes >= 0 && h >= 1 && w >= 1 && z_clip > 0.f);
  SGNN_CHECK_ARG(h <= 16384 && w <= 16384);      // 256 * pixel stays far below the snap limit of rule 4
  SGNN_CHECK_ARG((int64_t)ntri * 3 < ((int64_t)1 << 31) && (int64_t)nframes * h * w < ((int64_t)1 << 31));
  SGNN_CHECK_ARG(((uintptr_t)(COLOR ? (void *)keys : (void *)out) & 15) == 0);
  SGNN_CHECK_ARG(!COLOR || (((uintptr_t)out | (uintptr_t)rgba) & 3) == 0);
  if (nframes == 0) return SGNN_OK;
  SGNN_CHECK_ARG(out && frames && (ntri == 0 || (verts && faces)));
  SGNN_CHECK_ARG(!COLOR || (keys && rgba && (ntri == 0 || vcolors)));
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = (int64_t)nframes * h * w;
  const int64_t nwords = COLOR ? npix * 2 : npix;
  Pix<COLOR> *bits = COLOR ? reinterpret_cast<Pix<COLOR> *>(keys) : reinterpret_cast<Pix<COLOR> *>(out);
  SGNN_LAUNCH(k_render_clear<(COLOR ? 0xFFFFFFFFu : INF_BITS)>, dim3(sgnn_grid_for((nwords >> 2) + 4, 256, 8192)),
              dim3(256), 0, s, reinterpret_cast<uint32_t *>(bits), nwords);
  SGNN_CHECK_LAUNCH();
  if (ntri > 0) {
    if (status) {
      SGNN_LAUNCH(k_render_check, dim3(sgnn_grid_for((int64_t)ntri * 3, 256, 2048)), dim3(256), 0, s, faces,
                  (int64_t)ntri * 3, nverts, status);
      SGNN_CHECK_LAUNCH();
    }
    if (chunk <= 0 || chunk > nframes) chunk = nframes;
    if (wave_pixels <= 0) wave_pixels = WAVE_PIXELS_DEFAULT;
    for (int f0 = 0; f0 < nframes; f0 += chunk) {
      const int f1 = f0 + chunk < nframes ? f0 + chunk : nframes;
      const dim3 grid((ntri + 255) / 256, (f1 - f0 + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK);
      SGNN_CHECK_ARG(grid.y <= 65535);
      if (counters)
        SGNN_LAUNCH((k_render_triangles<true, COLOR>), grid, dim3(256), 0, s, verts, nverts, faces, ntri, frames, f0,
                    f1, h, w, z_clip, wave_pixels, bits, reinterpret_cast<unsigned long long *>(counters), vcolors);
      else
        SGNN_LAUNCH((k_render_triangles<false, COLOR>), grid, dim3(256), 0, s, verts, nverts, faces, ntri, frames, f0,
                    f1, h, w, z_clip, wave_pixels, bits, (unsigned long long *)nullptr, vcolors);
      SGNN_CHECK_LAUNCH();
    }
  }
  if constexpr (COLOR)
    SGNN_LAUNCH(k_rendercol_finish, dim3(sgnn_grid_for(npix, 256, 8192)), dim3(256), 0, s, keys, npix, depth_min,
                depth_max, reinterpret_cast<uint32_t *>(out), reinterpret_cast<uint32_t *>(rgba));
  else
    SGNN_LAUNCH(k_render_finish, dim3(sgnn_grid_for((npix >> 2) + 4, 256, 8192)), dim3(256), 0, s,
                reinterpret_cast<uint32_t *>(out), npix, depth_min, depth_max);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

}  // namespace

SGNN_EXPORT int sgnn_render_depth(const float *verts, int nverts, const int32_t *faces, int ntri,
                                  const sgnn_render_frame *frames, int nframes, int chunk, int h, int w, float z_clip,
                                  float depth_min, float depth_max, int wave_pixels, float *out, int32_t *status,
                                  int64_t *counters, sgnn_stream_t stream) {
  return render<false>(verts, nverts, faces, ntri, frames, nframes, chunk, h, w, z_clip, depth_min, depth_max,
                       wave_pixels, out, status, counters, nullptr, nullptr, nullptr, stream);
}

SGNN_EXPORT int sgnn_rendercol_draw(const float *verts, int nverts, const int32_t *faces, int ntri,
                                    const sgnn_render_frame *frames, int nframes, int chunk, int h, int w,
                                    float z_clip, float depth_min, float depth_max, int wave_pixels, float *out,
                                    int32_t *status, int64_t *counters, const uint8_t *vcolors, uint64_t *keys,
                                    uint8_t *rgba, sgnn_stream_t stream) {
  return render<true>(verts, nverts, faces, ntri, frames, nframes, chunk, h, w, z_clip, depth_min, depth_max,
                      wave_pixels, out, status, counters, vcolors, keys, rgba, stream);
}
