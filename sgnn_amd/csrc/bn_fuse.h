// BatchNorm statistics finalised inside the kernel that needs them (bn.hip: the small-level apply kernels; conv.hip: the
// small-level convolution that applies a folded BatchNormReLU to the rows it gathers).  Device code shared by both files so
// that the fp64 summation order — and with it mean / invstd — is the same bit for bit wherever the table is summed.
#pragma once
#include "common.h"

#define BN_FUSE_BLOCKS 4096
#define BN_FUSE_MAXC 64

// Small levels (few block partials, C <= BN_FUSE_MAXC): the apply kernels finalise the statistics themselves — every
// workgroup sums the short partial table in the same fixed order into LDS, workgroup 0 also stores the results the
// later passes / the caller need — and the separate finalize launch disappears.

struct BnFuse {
  const double *partial;   // NULL: statistics come from the mean/invstd (or coef) arrays
  int nblk;
  float eps, momentum;
  float *running_mean, *running_var, *save_mean, *save_invstd;   // forward
  float *dgamma, *dbeta;                                          // backward
};

// Per-channel totals of the block partials, computed by the whole workgroup: 256/c threads share a channel (strided
// partial sums), their pieces are added in thread order — a fixed order, identical in every workgroup.
// tot[0..c) = sum_a, tot[c..2c) = sum_b;  scratch: 512 doubles.  Contains two barriers.
// Round 6: what this costs is the NUMBER of dependent load rounds, ~0.75 us each (the table was written by the producing
// kernel's workgroups on all eight XCDs: every first touch misses this XCD's L2) — 6 rounds for the 684 16-row partials of a
// 11 k-row level with one 8-byte load per value and 8 blocks in flight (k_bn_apply 7.4 us there against 4.5 us on a 60 k-row
// level with 236 partials).  Even channel counts read two channels per 16-byte load and keep 32 loads in flight: the same
// table in 2 rounds.  The kernels that call this are the FUSE instantiations (small levels only), so the 64 + 64 registers
// cost the streaming instantiations nothing.  Any fixed order is a valid order: deterministic per (nblk, c).
#ifndef BN_TOTALS_WIDE
#define BN_TOTALS_WIDE 1     // 0: the one-value-per-load form everywhere (scripts/build_variant.sh A/B builds)
#endif
typedef double f64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void bn_fuse_totals(const BnFuse &f, int c, double *scratch, double *tot) {
  const int tid = threadIdx.x;
  const int tpc = 256 / c;                       // >= 4 for c <= BN_FUSE_MAXC
  if (BN_TOTALS_WIDE && (c & 1) == 0 && (((uintptr_t)f.partial) & 15) == 0) {
    // thread = (part, which, channel pair): sums `which` (0: sum_a, 1: sum_b) of channels 2 p, 2 p + 1 over blocks part, part + tpc, ...
    const int hp = c >> 1;
    const int p2 = tid % hp, which = (tid / hp) & 1, part = tid / c;
    f64x2 acc = {0.0, 0.0};
    if (part < tpc) {
      constexpr int U = 32;
      for (int blk = part; blk < f.nblk; blk += U * tpc) {
        f64x2 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int bi = blk + u * tpc;
          v[u] = bi < f.nblk ? *reinterpret_cast<const f64x2 *>(f.partial + ((size_t)bi * 2 + which) * c + 2 * p2) : f64x2{0.0, 0.0};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc += v[u];
      }
      scratch[which * 256 + part * c + 2 * p2] = acc[0];
      scratch[which * 256 + part * c + 2 * p2 + 1] = acc[1];
    }
  } else {
    const int ch = tid % c, part = tid / c;
    double a = 0.0, b = 0.0;
    if (part < tpc) {
      // eight independent loads in flight per thread; the additions keep their order, missing entries add an exact 0.0
      for (int blk = part; blk < f.nblk; blk += 8 * tpc) {
        double va[8], vb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int bi = blk + u * tpc;
          const bool ok = bi < f.nblk;
          va[u] = ok ? f.partial[((size_t)bi * 2 + 0) * c + ch] : 0.0;
          vb[u] = ok ? f.partial[((size_t)bi * 2 + 1) * c + ch] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          a += va[u];
          b += vb[u];
        }
      }
      scratch[part * c + ch] = a;
      scratch[256 + part * c + ch] = b;
    }
  }
  __syncthreads();
  if (tid < c) {
    double s1 = 0.0, s2 = 0.0;
    for (int p = 0; p < tpc; ++p) {
      s1 += scratch[p * c + tid];
      s2 += scratch[256 + p * c + tid];
    }
    tot[tid] = s1;
    tot[c + tid] = s2;
  }
  __syncthreads();
}

// The same totals in two halves, for a kernel that has independent memory traffic of its own to put between them (the
// folded small-level convolution: rule entries, gathers, weight fragments).  bn_totals_issue starts the loads of this
// thread's first BN_TOTALS_EARLY table entries; bn_totals_finish adds them and the rest of the thread's entries in the order
// of bn_fuse_totals (a thread's blocks ascending, absent entries an exact 0.0, then the parts in thread order), so tot[] is
// bit for bit what bn_fuse_totals leaves.  C: even, <= BN_FUSE_MAXC; the table 16-byte aligned (the wide form above).
// bn_totals_finish contains one barrier; the caller puts a second one between its own use of tot[] and the next writer.
#define BN_TOTALS_EARLY 16
template <int C>
struct BnTotalsEarly {
  f64x2 v[BN_TOTALS_EARLY];
};
template <int C>
__device__ __forceinline__ void bn_totals_issue(const BnFuse &f, BnTotalsEarly<C> &e) {
  static_assert((C & 1) == 0 && C <= BN_FUSE_MAXC, "wide form: two channels per 16-byte load");
  constexpr int tpc = 256 / C, hp = C / 2;
  const int tid = threadIdx.x;
  const int p2 = tid % hp, which = (tid / hp) & 1, part = tid / C;
#pragma unroll
  for (int u = 0; u < BN_TOTALS_EARLY; ++u) {
    const int bi = part + u * tpc;
    e.v[u] = (part < tpc && bi < f.nblk) ? *reinterpret_cast<const f64x2 *>(f.partial + ((size_t)bi * 2 + which) * C + 2 * p2)
                                          : f64x2{0.0, 0.0};
  }
}
template <int C>
__device__ __forceinline__ void bn_totals_finish(const BnFuse &f, const BnTotalsEarly<C> &e, double *scratch, double *tot) {
  constexpr int tpc = 256 / C, hp = C / 2, U = BN_TOTALS_EARLY;
  const int tid = threadIdx.x;
  const int p2 = tid % hp, which = (tid / hp) & 1, part = tid / C;
  if (part < tpc) {
    f64x2 acc = {0.0, 0.0};
#pragma unroll
    for (int u = 0; u < U; ++u) acc += e.v[u];
    for (int blk = part + U * tpc; blk < f.nblk; blk += U * tpc) {
      f64x2 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int bi = blk + u * tpc;
        v[u] = bi < f.nblk ? *reinterpret_cast<const f64x2 *>(f.partial + ((size_t)bi * 2 + which) * C + 2 * p2) : f64x2{0.0, 0.0};
      }
#pragma unroll
      for (int u = 0; u < U; ++u) acc += v[u];
    }
    scratch[which * 256 + part * C + 2 * p2] = acc[0];
    scratch[which * 256 + part * C + 2 * p2 + 1] = acc[1];
  }
  __syncthreads();
  if (tid < C) {
    double s1 = 0.0, s2 = 0.0;
    for (int p = 0; p < tpc; ++p) {
      s1 += scratch[p * C + tid];
      s2 += scratch[256 + p * C + tid];
    }
    tot[tid] = s1;
    tot[C + tid] = s2;
  }
}

// Finalising inside the apply kernels makes EVERY apply workgroup re-sum the partial table (L2-resident): worth it as
// long as that re-read stays small next to a separate launch (~5 us of GPU time + ~3 us of host time per finalize, ~70
// of them per training step).  Budget: 48 MB of partial reads per apply launch.
// (A finalise kernel made of ONE 1024-thread workgroup that reads the partial table in coalesced rows was measured against
//  the c single-channel workgroups of k_bn_finalize_fwd / _bwd: +3.8 us per launch inside the step, 6.64 vs 6.51 ms per step
//  — one CU cannot pull a 366 KB table as fast as 16 can; dropped.)
static inline bool bn_fuse_ok(int64_t nblk, int c, int64_t apply_grid) {
  return c <= BN_FUSE_MAXC && nblk <= BN_FUSE_BLOCKS && nblk * apply_grid * 2 * c * (int64_t)sizeof(double) <= (48ll << 20);
}

// What a convolution needs to apply a folded BatchNormReLU to the rows it gathers (conv.hip, planned by prog.hip): the
// BatchNorm's parameters and either the producer's partial table (training: fuse.partial != NULL; the forward kernel sums it
// and its workgroup 0 stores save_mean / save_invstd and updates the running statistics) or finished statistics (eval: the
// running statistics, which the forward kernel copies into save_mean / save_invstd; weight gradient: save_mean / save_invstd).
struct ConvPre {
  BnFuse fuse;
  const float *gamma, *beta;
  float leak;
  int64_t n_bn;              // rows of the BatchNorm's level (the convolution's input level): the statistics' divisor
  const int64_t *n_bn_dev;   // capacity mode: its device count (NULL: n_bn is exact)
};
