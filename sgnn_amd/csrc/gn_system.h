// The 32-double Gauss-Newton system of INTEGRATION.md section I rule 6 (and section R rule 7): what a lane adds for one
// association, how a block folds its lanes into one partial, the kernel that adds the partials, and the host tail
// that sizes the grid and launches that kernel.  track.hip and register.hip build their systems from this and differ
// in the residual alone.
//
// Every term is the product of two fp32 values and therefore exact in fp64; only the order of the additions is ours,
// and it is fixed: a lane's own terms in the order it meets them, an xor butterfly inside the wave, the four waves of a
// block through LDS in wave order, the blocks in index order.  No floating-point atomics, the same bits on every call.
#pragma once
#include "common.h"

constexpr int GN_BLOCK = 256;   // lanes per block of a system kernel: four waves
constexpr int GN_NSUM = 28;     // 21 of J^T J (upper triangle, row-major), 6 of J^T r, r^2
constexpr int GN_ENTRIES = 32;  // the sums, N, three zeros

__device__ __forceinline__ double gn_wave_allsum(double v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);             // every lane ends with the same bits
  return v;
}

// J[0..5]: the row of the Jacobian, J[6]: the residual; all zeros for a lane without an association
__device__ __forceinline__ void gn_accumulate(double (&acc)[GN_NSUM], const float (&J)[7]) {
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) acc[k++] += (double)J[a] * (double)J[b];
#pragma unroll
  for (int a = 0; a < 7; ++a) acc[21 + a] += (double)J[a] * (double)J[6];
}

// The block's 32 doubles to `out`; part is the block's LDS, [4][GN_ENTRIES].  Every lane of the block calls this.
__device__ __forceinline__ void gn_block_reduce(double (&acc)[GN_NSUM], int count, double (*part)[GN_ENTRIES],
                                                double *__restrict__ out) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int k = 0; k < GN_NSUM; ++k) acc[k] = gn_wave_allsum(acc[k]);
  const double n = gn_wave_allsum((double)count);                       // integers: exact
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < GN_NSUM; ++k) part[wave][k] = acc[k];
    part[wave][28] = n;
    part[wave][29] = part[wave][30] = part[wave][31] = 0.0;
  }
  __syncthreads();
  if (threadIdx.x < GN_ENTRIES) {
    const int t = (int)threadIdx.x;
    out[t] = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
  }
}

// the partials of one record in index order; one block of 64 per record, thread t owns entry t of the 32
static __global__ __launch_bounds__(64) void k_gn_finish(const double *__restrict__ ws, int nblk,
                                                        double *__restrict__ out) {
  const int t = (int)threadIdx.x;
  if (t >= GN_ENTRIES) return;
  const double *p = ws + (int64_t)blockIdx.x * nblk * GN_ENTRIES + t;
  double s = p[0];
  for (int b = 1; b < nblk; ++b) s += p[(int64_t)b * GN_ENTRIES];
  out[(int64_t)blockIdx.x * GN_ENTRIES + t] = s;
}

// What the sgnn_*_system entry points share once their own arguments are checked: nblk = min(ceil(n / GN_BLOCK),
// max_blocks), a function of n alone; the workspace check; `system(nblk)`, the caller's launch of its system kernel on
// a (nblk, npairs) grid; k_gn_finish.
template <class SystemLaunch>
static inline int gn_launch(int64_t n, int max_blocks, int npairs, void *ws, int64_t ws_bytes, double *out,
                            hipStream_t s, SystemLaunch system) {
  const int64_t want = (n + GN_BLOCK - 1) / GN_BLOCK;
  const int nblk = (int)(want < max_blocks ? want : max_blocks);
  SGNN_CHECK_ARG(ws_bytes >= (int64_t)npairs * nblk * GN_ENTRIES * (int64_t)sizeof(double));
  system(nblk);
  SGNN_CHECK_LAUNCH();
  SGNN_LAUNCH(k_gn_finish, dim3(npairs), dim3(64), 0, s, (const double *)ws, nblk, out);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
