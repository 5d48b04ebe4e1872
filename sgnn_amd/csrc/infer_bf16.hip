// bf16 inference kernels: the forward pass of a program in the bf16 inference layout (sgnn_prog_forward with
// training = 2 | 4, prog.hip).  Feature rows are stored as bf16 with a row stride (`ld`, elements) that is a multiple of
// 8, so that a row chunk of 8 channels is one 16-byte load; math runs in fp32 and rounds once at the store.
//
// Pad columns [c, ld) of a row are never written and, in the liveness-packed inference arena, hold whatever an earlier
// buffer left there (NaN patterns included).  Every kernel that reads whole 16-byte chunks therefore zeroes the channels
// >= c in registers before they meet a weight (NaN * 0 = NaN: zero weights alone are not enough).
//
// The convolution is the counterpart of conv.hip's output-stationary rulebook walk (offset-major int32 table[K][ld],
// -1 = no rule, XCD-aware workgroup order), contracted with v_mfma_f32_16x16x32_bf16.  Its k dimension is the flattened
// (offset, 8-channel chunk) list: chunk t = offset * CB + chunk, CB = ceil(cin / 8), and lane quarter q of k-block b holds
// chunk 4b + q — so one MFMA contracts two offsets of a 16-channel layer, four of an 8-channel one, and every lane issues
// one 16-byte gather per MFMA.  Weights (fp32 parameters) are rounded to bf16 once per call into the B-fragment order.
#include <stdint.h>
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

namespace {

// fp32 -> bf16, round to nearest even (NaN stays NaN): the rounding torch's .to(torch.bfloat16) applies
__device__ __forceinline__ uint16_t f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void *p, uint64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)(uint32_t)bytes, 0x00020000);
}

// zero the bf16 elements j >= nv of an 8-element chunk (nv may be <= 0 or >= 8)
__device__ __forceinline__ uint4 mask_chunk(uint4 v, int nv) {
  auto mw = [&](int w) -> uint32_t {
    const int keep = nv - 2 * w;
    return keep >= 2 ? 0xffffffffu : (keep == 1 ? 0x0000ffffu : 0u);
  };
  v.x &= mw(0);
  v.y &= mw(1);
  v.z &= mw(2);
  v.w &= mw(3);
  return v;
}

struct BConv {
  const uint16_t *x;          // bf16 rows, row stride ldx elements
  int64_t n_in, ldx;
  int cin;
  const uint4 *wf;            // B fragments: [groups][NB][NT][64 lanes] x 8 bf16
  const int32_t *table;       // [table_rows][ld]
  int64_t ld;
  int K;
  int64_t n_out;
  uint16_t *y;                // output row (row * groups + group), stride ldy elements
  int64_t ldy;
  int cout;
  const uint16_t *addend;     // optional bf16 residual, stride ld_add
  int64_t ld_add;
  const int32_t *kmap;        // optional: offset k of group g reads table row kmap[g * K + k]
  int groups, table_rows;
  const int64_t *n_dev;       // capacity mode: live output rows on the device
};

constexpr int BLK_KIB = 32;   // B fragments staged at a time: BLK_KIB / NT k-blocks of NT KiB each

template <int CB, int NT, int M>
__global__ __launch_bounds__(256) void k_conv_fwd_bf16(BConv p) {
  constexpr int RPW = 16 * M;                // rows per wave
  constexpr int NBC = BLK_KIB / NT;          // k-blocks per staged chunk
  __shared__ uint4 wl[NBC * NT * 64];
  __shared__ int32_t kmap_s[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int64_t n_out = sgnn_dyn_n(p.n_out, p.n_dev);
  const unsigned groups = (unsigned)p.groups;
  const unsigned nwg = (unsigned)((n_out + 4 * RPW - 1) / (4 * RPW)) * groups;
  if (blockIdx.x >= nwg) return;             // past the live rows (capacity mode): uniform over the workgroup
  // all groups of a row tile run next to each other, tiles in contiguous ranges per XCD (they gather the same rows)
  const unsigned lin = sgnn_xcd_tile(blockIdx.x, nwg);
  const unsigned tile = lin / groups, grp = lin % groups;
  const int64_t row0 = ((int64_t)tile * 4 + wave) * RPW;
  const int K = p.K, NB = (K * CB + 3) / 4;
  if (tid < K) kmap_s[tid] = p.kmap ? p.kmap[grp * K + tid] : tid;
  const uint4 *wf = p.wf + (size_t)grp * NB * NT * 64;
  const __amdgpu_buffer_rsrc_t rs_x = rsrc(p.x, (uint64_t)((p.n_in - 1) * p.ldx + 8 * CB) * 2u);
  const __amdgpu_buffer_rsrc_t rs_t = rsrc(p.table, (uint64_t)p.table_rows * p.ld * 4u);
  const uint32_t ldx2 = (uint32_t)p.ldx * 2u;

  f32x4 acc[M][NT];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[m][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // rule entries of this lane's chunk in k-block b, for its row in each of the M tiles (-1: no rule / no chunk)
  auto load_idx = [&](int b, int32_t (&iv)[M]) {
    const int t = 4 * b + q, o = t / CB;
    const int trow = o < K ? kmap_s[o] : -1;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const uint32_t off = trow < 0 ? 0u : (uint32_t)(trow * p.ld + row0 + m * 16 + r) * 4u;
      const int32_t v = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_t, off, 0, 0);
      iv[m] = trow < 0 ? -1 : v;
    }
  };
  auto gather = [&](int b, const int32_t (&iv)[M], uint4 (&a)[M]) {
    const int ch = (4 * b + q) % CB;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const uint32_t off = iv[m] < 0 ? 0xffffffffu : (uint32_t)iv[m] * ldx2 + (uint32_t)ch * 16u;
      const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs_x, off, 0, 0);
      a[m] = uint4{v.x, v.y, v.z, v.w};
    }
  };
  auto mma = [&](int b, int bb, uint4 (&a)[M]) {
    const int nv = p.cin - 8 * ((4 * b + q) % CB);   // live channels of this lane's chunk (pad columns -> 0)
    uint4 bw[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) bw[nt] = wl[(bb * NT + nt) * 64 + lane];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const bf16x8 av = __builtin_bit_cast(bf16x8, mask_chunk(a[m], nv));
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, __builtin_bit_cast(bf16x8, bw[nt]), acc[m][nt], 0, 0, 0);
    }
  };

  for (int b0 = 0; b0 < NB; b0 += NBC) {
    const int nbc = (NB - b0) < NBC ? (NB - b0) : NBC;
    __syncthreads();                                      // (also publishes kmap_s)
    for (int e = tid; e < nbc * NT * 64; e += 256) wl[e] = wf[(size_t)b0 * NT * 64 + e];
    __syncthreads();
    // rule entries two k-blocks ahead, gathered rows one ahead; loads past the chunk are clamped to its last block
    // (issued unconditionally so that every wait is a counted one) and their rows dropped
    int32_t i1[M], i2[M];
    uint4 a0[M], a1[M];
    load_idx(b0, i1);
    gather(b0, i1, a0);
    load_idx(b0 + (nbc > 1 ? 1 : 0), i1);
    for (int bb = 0; bb < nbc; ++bb) {
      load_idx(b0 + (bb + 2 < nbc ? bb + 2 : nbc - 1), i2);
      gather(b0 + (bb + 1 < nbc ? bb + 1 : nbc - 1), i1, a1);
      __builtin_amdgcn_sched_barrier(0);
      mma(b0 + bb, bb, a0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        a0[m] = a1[m];
        i1[m] = i2[m];
      }
    }
  }

#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = row0 + m * 16 + q * 4 + i;
        const int col = nt * 16 + r;
        if (row >= n_out || col >= p.cout) continue;
        const int64_t orow = row * groups + grp;
        float v = acc[m][nt][i];
        if (p.addend) v += bf2f(p.addend[orow * p.ld_add + col]);
        p.y[orow * p.ldy + col] = f2bf(v);
      }
}

// any (cin, cout): one thread per output element, fp32 FMA over bf16 operands.  Keeps the mode total for widths
// outside the MFMA instantiations (cin or cout > 64); not a performance path.
__global__ __launch_bounds__(256) void k_conv_fwd_bf16_generic(BConv p, const float *__restrict__ w) {
  const int64_t n_out = sgnn_dyn_n(p.n_out, p.n_dev);
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_out * p.groups * p.cout) return;
  const int64_t orow = t / p.cout;
  const int n = (int)(t - orow * p.cout);
  const int64_t row = orow / p.groups;
  const int grp = (int)(orow - row * p.groups);
  w += (int64_t)grp * p.K * p.cin * p.cout;
  float acc = 0.f;
  for (int k = 0; k < p.K; ++k) {
    const int32_t idx = p.table[(int64_t)(p.kmap ? p.kmap[grp * p.K + k] : k) * p.ld + row];
    if (idx < 0) continue;
    const uint16_t *xr = p.x + (int64_t)idx * p.ldx;
    for (int c = 0; c < p.cin; ++c) acc = fmaf(bf2f(xr[c]), bf2f(f2bf(w[((int64_t)k * p.cin + c) * p.cout + n])), acc);
  }
  if (p.addend) acc += bf2f(p.addend[orow * p.ld_add + n]);
  p.y[orow * p.ldy + n] = f2bf(acc);
}

// B fragments of the MFMA kernel from fp32 weights [groups][K][cin][cout]: block b, column tile nt, lane l holds
// W[offset][channel][nt * 16 + (l & 15)] for chunk t = 4b + (l >> 4) (offset t / CB, channels 8 (t % CB) + 0..7); zero
// outside the filter
__global__ __launch_bounds__(256) void k_bf16_wfrag(const float *__restrict__ w, int K, int cin, int cout, int CB, int NB,
                                                    int NT, int groups, uint4 *__restrict__ wf) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)groups * NB * NT * 64) return;
  const int lane = (int)(t & 63);
  const int64_t u = t >> 6;
  const int nt = (int)(u % NT), b = (int)((u / NT) % NB), g = (int)(u / ((int64_t)NT * NB));
  const int tt = 4 * b + (lane >> 4), o = tt / CB, ch = tt % CB, n = nt * 16 + (lane & 15);
  uint32_t h[4];
  for (int j2 = 0; j2 < 4; ++j2) {
    uint32_t pair = 0;
    for (int e = 0; e < 2; ++e) {
      const int c = 8 * ch + 2 * j2 + e;
      const float v = (o < K && c < cin && n < cout) ? w[(((int64_t)g * K + o) * cin + c) * cout + n] : 0.f;
      pair |= (uint32_t)f2bf(v) << (16 * e);
    }
    h[j2] = pair;
  }
  wf[t] = uint4{h[0], h[1], h[2], h[3]};
}

// ---- row ops (one thread per element; rows r, channels c; bf16 stride ld* in elements) ----
#define ELEM_LOOP(total)                                                                            \
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x, stride_ = (int64_t)gridDim.x * 256; \
       g < (total); g += stride_)

__global__ __launch_bounds__(256) void k_bn_eval_bf16(const uint16_t *__restrict__ x, int64_t ldx, int64_t n, int c,
                                                      const float *__restrict__ gamma, const float *__restrict__ beta,
                                                      const float *__restrict__ rmean, const float *__restrict__ rvar,
                                                      float eps, float leak, uint16_t *__restrict__ y, int64_t ldy,
                                                      const int64_t *n_dev) {
  n = sgnn_dyn_n(n, n_dev);
  ELEM_LOOP(n * c) {
    const int64_t r = g / c;
    const int ch = (int)(g - r * c);
    const float invstd = 1.0f / sqrtf(rvar[ch] + eps);     // as k_bn_eval_stats (bn.hip)
    y[r * ldy + ch] = f2bf(sgnn_bn_act(bf2f(x[r * ldx + ch]), rmean[ch], invstd, gamma ? gamma[ch] : 1.f,
                                       beta ? beta[ch] : 0.f, leak));
  }
}

__global__ __launch_bounds__(256) void k_gather_rows_bf16(const uint16_t *__restrict__ x, int64_t ldx, int c,
                                                          const int32_t *__restrict__ idx, int64_t m,
                                                          uint16_t *__restrict__ y, int64_t ldy, const int64_t *n_dev) {
  m = sgnn_dyn_n(m, n_dev);
  ELEM_LOOP(m * c) {
    const int64_t r = g / c;
    const int ch = (int)(g - r * c);
    const int32_t i = idx[r];
    y[r * ldy + ch] = i >= 0 ? x[(int64_t)i * ldx + ch] : (uint16_t)0;
  }
}

__global__ __launch_bounds__(256) void k_add_bf16(const uint16_t *__restrict__ a, int64_t lda, const uint16_t *__restrict__ b,
                                                  int64_t ldb, int64_t n, int c, uint16_t *y, int64_t ldy,
                                                  const int64_t *n_dev) {
  n = sgnn_dyn_n(n, n_dev);
  ELEM_LOOP(n * c) {
    const int64_t r = g / c;
    const int ch = (int)(g - r * c);
    y[r * ldy + ch] = f2bf(bf2f(a[r * lda + ch]) + bf2f(b[r * ldb + ch]));
  }
}

__global__ __launch_bounds__(256) void k_join_bf16(const uint16_t *__restrict__ a, int64_t lda, int ca,
                                                   const uint16_t *__restrict__ b, int64_t ldb, int cb, int64_t n,
                                                   uint16_t *__restrict__ y, int64_t ldy, const int64_t *n_dev) {
  n = sgnn_dyn_n(n, n_dev);
  const int c = ca + cb;
  ELEM_LOOP(n * c) {
    const int64_t r = g / c;
    const int ch = (int)(g - r * c);
    y[r * ldy + ch] = ch < ca ? a[r * lda + ch] : b[r * ldb + ch - ca];
  }
}

struct Cat3F {
  const float *src[3];
  const int32_t *idx[3];
  int c[3];
};

// fp32 sources (contiguous rows, optional row index arrays, -1 = zeros) -> one bf16 row of c0 + c1 + c2 channels
__global__ __launch_bounds__(256) void k_concat3_bf16(Cat3F s, int64_t m, uint16_t *__restrict__ y, int64_t ldy,
                                                      const int64_t *n_dev) {
  m = sgnn_dyn_n(m, n_dev);
  const int c01 = s.c[0] + s.c[1], c = c01 + s.c[2];
  ELEM_LOOP(m * c) {
    const int64_t r = g / c;
    const int col = (int)(g - r * c);
    const int which = col < s.c[0] ? 0 : (col < c01 ? 1 : 2);
    const int lc = col - (which == 0 ? 0 : (which == 1 ? s.c[0] : c01));
    const int64_t i = s.idx[which] ? (int64_t)s.idx[which][r] : r;
    y[r * ldy + col] = f2bf(i >= 0 ? s.src[which][i * s.c[which] + lc] : 0.f);
  }
}

#define LIN_MAX 4
struct LinHeads {
  const float *w[LIN_MAX], *b[LIN_MAX];
};

// per-site heads: bf16 rows in, fp32 logits out (contiguous [n][cout])
__global__ __launch_bounds__(256) void k_linear_bf16(const uint16_t *__restrict__ x, int64_t ldx, int64_t n, int cin,
                                                     LinHeads h, int cout, float *__restrict__ y, const int64_t *n_dev) {
  n = sgnn_dyn_n(n, n_dev);
  ELEM_LOOP(n * cout) {
    const int64_t r = g / cout;
    const int o = (int)(g - r * cout);
    const uint16_t *xr = x + r * ldx;
    const float *w = h.w[o];
    float acc = 0.f;
    for (int c = 0; c < cin; ++c) acc = fmaf(bf2f(xr[c]), w[c], acc);
    y[g] = acc + (h.b[o] ? h.b[o][0] : 0.f);
  }
}

__global__ __launch_bounds__(256) void k_bf16_to_f32(const uint16_t *__restrict__ x, int64_t ldx, int64_t n, int c,
                                                     float *__restrict__ y, const int64_t *n_dev) {
  n = sgnn_dyn_n(n, n_dev);
  ELEM_LOOP(n * c) {
    const int64_t r = g / c;
    y[g] = bf2f(x[r * ldx + (g - r * c)]);
  }
}

template <int CB, int NT>
void launch_cbnt(const BConv &p, bool small, hipStream_t s) {
  if (small) {
    const unsigned grid = (unsigned)((p.n_out + 63) / 64) * (unsigned)p.groups;
    SGNN_LAUNCH((k_conv_fwd_bf16<CB, NT, 1>), dim3(grid), dim3(256), 0, s, p);
  } else {
    const unsigned grid = (unsigned)((p.n_out + 255) / 256) * (unsigned)p.groups;
    SGNN_LAUNCH((k_conv_fwd_bf16<CB, NT, 4>), dim3(grid), dim3(256), 0, s, p);
  }
}
typedef void (*LaunchFn)(const BConv &, bool, hipStream_t);
#define ROW(CB) {launch_cbnt<CB, 1>, launch_cbnt<CB, 2>, launch_cbnt<CB, 3>, launch_cbnt<CB, 4>}
const LaunchFn g_launch[8][4] = {ROW(1), ROW(2), ROW(3), ROW(4), ROW(5), ROW(6), ROW(7), ROW(8)};
#undef ROW

inline bool mfma_shape(int cin, int cout) { return cin >= 1 && cin <= 64 && cout >= 1 && cout <= 64; }
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace

// bytes of the bf16 B fragments of a (groups x K x cin x cout) filter; 0 when the generic kernel runs (it reads the
// fp32 weights directly)
int64_t sgnn_bf16_wfrag_bytes(int cin, int cout, int K, int groups) {
  if (!mfma_shape(cin, cout)) return 0;
  const int64_t nb = ceil_div((int64_t)K * ceil_div(cin, 8), 4);
  return ((int64_t)groups * nb * ceil_div(cout, 16) * 64 * 16 + 255) & ~int64_t(255);
}

// weights -> fragments (into wf, sgnn_bf16_wfrag_bytes); nothing for shapes of the generic kernel
int sgnn_bf16_conv_prepare(const float *w, int cin, int cout, int K, int groups, void *wf, sgnn_stream_t stream) {
  if (!mfma_shape(cin, cout)) return SGNN_OK;
  SGNN_CHECK_ARG(w && wf);
  const int CB = (cin + 7) / 8, NT = (cout + 15) / 16, NB = (K * CB + 3) / 4;
  const int64_t total = (int64_t)groups * NB * NT * 64;
  SGNN_LAUNCH(k_bf16_wfrag, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, w, K, cin, cout, CB,
              NB, NT, groups, (uint4 *)wf);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

// the convolution itself, on prepared fragments (w: the fp32 weights, read by the generic kernel only)
int sgnn_bf16_conv_run(const void *x, int64_t n_in, int cin, int64_t ldx, const float *w, const void *wf, int K,
                       const int32_t *table, int64_t ld, int64_t n_out, int cout, void *y, int64_t ldy,
                       const void *addend, int64_t ld_add, const int32_t *kmap, int groups, int table_rows,
                       const int64_t *n_dev, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(cin >= 1 && cout >= 1 && K >= 1 && K <= 64 && n_out >= 0 && ld >= n_out && groups >= 1 && groups <= 64 &&
                 table_rows >= 1 && table_rows <= 64 && (kmap || table_rows >= K) && ldx >= cin && ldy >= cout &&
                 (!addend || ld_add >= cout));
  if (n_out == 0) return SGNN_OK;
  SGNN_CHECK_ARG(x && w && table && y && n_in >= 1);
  SGNN_CHECK_ARG(ld % 256 == 0);   // and table[k][n_out..roundup256(n_out)) must be -1 (as for sgnn_conv_fwd)
  if ((n_in * ldx + 64) * 2 > 0xFFFFF000ll || (int64_t)table_rows * ld * 4 > 0xFFFFF000ll) {
    sgnn_set_error("sgnn_bf16_conv: a slab exceeds the 4 GiB raw-buffer window (n_in=%lld, n_out=%lld)", (long long)n_in,
                   (long long)n_out);
    return SGNN_EOVERFLOW;
  }
  const BConv p{(const uint16_t *)x, n_in, ldx, cin, (const uint4 *)wf, table, ld, K, n_out, (uint16_t *)y, ldy, cout,
                (const uint16_t *)addend, ld_add, kmap, groups, table_rows, n_dev};
  hipStream_t s = (hipStream_t)stream;
  const int prof = sgnn_prof_begin_launch(0, n_out * groups, cin, cout, K, 0, s);
  if (mfma_shape(cin, cout)) {
    SGNN_CHECK_ARG(wf && (ldx & 1) == 0 && ((uintptr_t)x & 3) == 0);   // 16-byte chunk loads need dword alignment
    // below sgnn_tune.conv_small_rows the 16-row tiles (64 per workgroup) fill more of the chip
    const bool small = n_out < g_tune.conv_small_rows;
    g_launch[(cin + 7) / 8 - 1][(cout + 15) / 16 - 1](p, small, s);
  } else {
    const int64_t total = n_out * groups * cout;
    SGNN_LAUNCH(k_conv_fwd_bf16_generic, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, p, w);
  }
  sgnn_prof_end_launch(prof, s);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

extern "C" int sgnn_expand_weights(const float *w, int cin, int cout, float *wc, sgnn_stream_t stream);   // conv.hip

SGNN_EXPORT int64_t sgnn_bf16_conv_ws_bytes(int cin, int cout, int K, int expand) {
  if (expand) return ((64 * (int64_t)cin * cout * 4 + 255) & ~int64_t(255)) + sgnn_bf16_wfrag_bytes(cin, cout, 8, 8);
  return sgnn_bf16_wfrag_bytes(cin, cout, K, 1);
}

SGNN_EXPORT int sgnn_bf16_conv_fwd(const void *x, int64_t n_in, int cin, int64_t ldx, const float *w, int K,
                                   const int32_t *table, int64_t ld, int64_t n_out, int cout, void *y, int64_t ldy,
                                   const void *addend, int64_t ld_add, const int64_t *n_dev, void *ws, int64_t ws_bytes,
                                   sgnn_stream_t stream) {
  SGNN_CHECK_ARG(ws_bytes >= sgnn_bf16_conv_ws_bytes(cin, cout, K, 0) && (ws || ws_bytes == 0));
  const int rc = sgnn_bf16_conv_prepare(w, cin, cout, K, 1, ws, stream);
  if (rc != SGNN_OK) return rc;
  return sgnn_bf16_conv_run(x, n_in, cin, ldx, w, ws, K, table, ld, n_out, cout, y, ldy, addend, ld_add, nullptr, 1, K,
                            n_dev, stream);
}

// the 8-child up-sampling convolution (OP_EXPAND): parent rows in, child rows 8p + parity out, 3x3x3 weights w
int sgnn_bf16_conv_expand_impl(const void *x, int64_t n, int cin, int64_t ldx, const float *w, const int32_t *nbr,
                               int64_t ld, int cout, void *y, int64_t ldy, const int64_t *n_dev, void *ws,
                               sgnn_stream_t stream) {
  const int32_t *S, *ST, *PAR;
  int rc = sgnn_expand_maps(&S, &ST, &PAR);
  if (rc != SGNN_OK) return rc;
  float *wc = (float *)ws;
  void *wf = (char *)ws + ((64 * (int64_t)cin * cout * 4 + 255) & ~int64_t(255));
  if ((rc = sgnn_expand_weights(w, cin, cout, wc, stream)) != SGNN_OK) return rc;
  if ((rc = sgnn_bf16_conv_prepare(wc, cin, cout, 8, 8, wf, stream)) != SGNN_OK) return rc;
  return sgnn_bf16_conv_run(x, n, cin, ldx, wc, wf, 8, nbr, ld, n, cout, y, ldy, nullptr, 0, S, 8, 27, n_dev, stream);
}

SGNN_EXPORT int sgnn_bf16_conv_expand(const void *x, int64_t n, int cin, int64_t ldx, const float *w, const int32_t *nbr,
                                      int64_t ld, int cout, void *y, int64_t ldy, const int64_t *n_dev, void *ws,
                                      int64_t ws_bytes, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(ws && ws_bytes >= sgnn_bf16_conv_ws_bytes(cin, cout, 27, 1));
  return sgnn_bf16_conv_expand_impl(x, n, cin, ldx, w, nbr, ld, cout, y, ldy, n_dev, ws, stream);
}

SGNN_EXPORT int sgnn_bf16_bn_eval(const void *x, int64_t ldx, int64_t n, int c, const float *gamma, const float *beta,
                                  const float *running_mean, const float *running_var, float eps, float leak, void *y,
                                  int64_t ldy, const int64_t *n_dev, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && c >= 1 && ldx >= c && ldy >= c);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(x && y && running_mean && running_var);
  SGNN_LAUNCH(k_bn_eval_bf16, dim3(sgnn_grid_for(n * c, 256)), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)x, ldx, n,
              c, gamma, beta, running_mean, running_var, eps, leak, (uint16_t *)y, ldy, n_dev);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_bf16_gather_rows(const void *x, int64_t ldx, int c, const int32_t *idx, int64_t m, void *y, int64_t ldy,
                                      const int64_t *n_dev, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(m >= 0 && c >= 1 && ldx >= c && ldy >= c);
  if (m == 0) return SGNN_OK;
  SGNN_CHECK_ARG(x && y && idx);
  SGNN_LAUNCH(k_gather_rows_bf16, dim3(sgnn_grid_for(m * c, 256)), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)x,
              ldx, c, idx, m, (uint16_t *)y, ldy, n_dev);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_bf16_add(const void *a, int64_t lda, const void *b, int64_t ldb, int64_t n, int c, void *y, int64_t ldy,
                              const int64_t *n_dev, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && c >= 1 && lda >= c && ldb >= c && ldy >= c);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(a && b && y);
  SGNN_LAUNCH(k_add_bf16, dim3(sgnn_grid_for(n * c, 256)), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)a, lda,
              (const uint16_t *)b, ldb, n, c, (uint16_t *)y, ldy, n_dev);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_bf16_join(const void *a, int64_t lda, int ca, const void *b, int64_t ldb, int cb, int64_t n, void *y,
                               int64_t ldy, const int64_t *n_dev, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && ca >= 1 && cb >= 1 && lda >= ca && ldb >= cb && ldy >= ca + cb);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(a && b && y);
  SGNN_LAUNCH(k_join_bf16, dim3(sgnn_grid_for(n * (ca + cb), 256)), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)a,
              lda, ca, (const uint16_t *)b, ldb, cb, n, (uint16_t *)y, ldy, n_dev);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_bf16_concat3(const float *a, int ca, const int32_t *ia, const float *b, int cb, const int32_t *ib,
                                  const float *c3, int cc, const int32_t *ic, int64_t m, void *y, int64_t ldy,
                                  const int64_t *n_dev, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(m >= 0 && ca >= 0 && cb >= 0 && cc >= 0 && ca + cb + cc >= 1 && ldy >= ca + cb + cc);
  SGNN_CHECK_ARG((!ca || a) && (!cb || b) && (!cc || c3));
  if (m == 0) return SGNN_OK;
  SGNN_CHECK_ARG(y);
  const Cat3F s{{a, b, c3}, {ia, ib, ic}, {ca, cb, cc}};
  SGNN_LAUNCH(k_concat3_bf16, dim3(sgnn_grid_for(m * (ca + cb + cc), 256)), dim3(256), 0, (hipStream_t)stream, s, m,
              (uint16_t *)y, ldy, n_dev);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

int sgnn_bf16_linear_rows(const void *x, int64_t ldx, int64_t n, int cin, const float *const *w, const float *const *b,
                          int cout, float *y, const int64_t *n_dev, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && cin >= 1 && ldx >= cin && cout >= 1 && cout <= LIN_MAX);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(x && y && w);
  LinHeads h{};
  for (int o = 0; o < cout; ++o) {
    SGNN_CHECK_ARG(w[o]);
    h.w[o] = w[o];
    h.b[o] = b ? b[o] : nullptr;
  }
  SGNN_LAUNCH(k_linear_bf16, dim3(sgnn_grid_for(n * cout, 256)), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)x, ldx,
              n, cin, h, cout, y, n_dev);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}

SGNN_EXPORT int sgnn_bf16_linear(const void *x, int64_t ldx, int64_t n, int cin, const float *w, const float *bias, int cout,
                                 float *y, const int64_t *n_dev, sgnn_stream_t stream) {
  SGNN_CHECK_ARG(cout >= 1 && cout <= LIN_MAX && w);
  const float *wr[LIN_MAX] = {}, *br[LIN_MAX] = {};
  for (int o = 0; o < cout; ++o) {
    wr[o] = w + (int64_t)o * cin;
    br[o] = bias ? bias + o : nullptr;
  }
  return sgnn_bf16_linear_rows(x, ldx, n, cin, wr, br, cout, y, n_dev, stream);
}

SGNN_EXPORT int sgnn_bf16_to_f32(const void *x, int64_t ldx, int64_t n, int c, float *y, const int64_t *n_dev,
                                 sgnn_stream_t stream) {
  SGNN_CHECK_ARG(n >= 0 && c >= 1 && ldx >= c);
  if (n == 0) return SGNN_OK;
  SGNN_CHECK_ARG(x && y);
  SGNN_LAUNCH(k_bf16_to_f32, dim3(sgnn_grid_for(n * c, 256)), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)x, ldx, n,
              c, y, n_dev);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
