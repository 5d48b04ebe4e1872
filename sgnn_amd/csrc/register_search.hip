// Candidate transforms scored against an integer distance field (sgnn_amd.register.search): the piece that produces
// the guesses register.align polishes.  Every candidate moves one shared point set into the grid of a squared-distance
// volume (edt's dist2 of the destination's surface voxels), rounds each position to its voxel and adds up the capped
// squared distances.  Every result is an integer, so no bit depends on the launch or on the order of the additions.  The
// rules are listed in INTEGRATION.md section X; that text is the contract, and tests/register_search_ref.py restates it
// independently in NumPy.
//
// Kernels:
//   k_register_score  a lane per candidate, grid = (blocks of 256 candidates, slices of the points).  The 12 floats of
//                     a lane's record stay in registers; the block stages a tile of 256 points in LDS and every lane
//                     reads the same point at the same time, an LDS broadcast.  A lane holds its three sums, so there
//                     is no cross-lane reduction.  Neighbouring lanes are neighbouring candidates: on the level-0
//                     lattice they differ by one pitch along x and their gathers fall into a few cache lines of one
//                     row of the volume.  A slice adds its sums to the output with 64-bit integer atomics; the entry
//                     point zeroes the output first.
//
// Built with -ffp-contract=off (Makefile): every product and sum is rounded on its own.
#include <math.h>
#include "common.h"
#include "geom.h"

namespace {

constexpr int BLOCK = 256;          // candidates per block
constexpr int TILE = 256;           // points per LDS tile: one per thread when it is filled
constexpr int TARGET_BLOCKS = 2048; // the points are sliced until the grid has about this many blocks (8 per CU)

__global__ __launch_bounds__(BLOCK) void k_register_score(const float *__restrict__ points, int npts,
                                                         const int32_t *__restrict__ dist2, int dx, int dy, int dz,
                                                         const sgnn_register_pose *__restrict__ poses, int nposes,
                                                         int cap2, int inlier2,
                                                         unsigned long long *__restrict__ out) {
  __shared__ float tile[TILE][4];   // x, y, z and a pad: one 16-byte broadcast read per point
  const int64_t b = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = b < nposes;
  float m[12];
  {
    const float *src = poses[live ? b : 0].m;       // a lane past the end scores record 0 and writes nothing
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = src[k];
  }
  const bool rec_ok = m[0] == m[0];                 // non-finite record (the host stores NaN): every point outside
  const float hx = (float)(dx - 1), hy = (float)(dy - 1), hz = (float)(dz - 1);
  long long cost = 0;
  int inliers = 0, outside = 0;
  const int ntiles = (npts + TILE - 1) / TILE;      // npts < 2^31 - 65536: no overflow
  for (int t = (int)blockIdx.y; t < ntiles; t += (int)gridDim.y) {
    const int64_t p0 = (int64_t)t * TILE;
    const int n = (int)min((int64_t)TILE, (int64_t)npts - p0);
    __syncthreads();                                // the tile of the round before has been read
    if ((int)threadIdx.x < n) {
      const float *p = points + (p0 + threadIdx.x) * 3;
      tile[threadIdx.x][0] = p[0], tile[threadIdx.x][1] = p[1], tile[threadIdx.x][2] = p[2];
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
      const float x = tile[j][0], y = tile[j][1], z = tile[j][2];
      // rule 2, rule 3: the comparison is made in float, so a NaN or a huge position never becomes an index
      const float nx = floorf(tsdf_affine_row(m, 0, x, y, z) + 0.5f);
      const float ny = floorf(tsdf_affine_row(m, 1, x, y, z) + 0.5f);
      const float nz = floorf(tsdf_affine_row(m, 2, x, y, z) + 0.5f);
      const bool in = rec_ok && nx >= 0.f && nx <= hx && ny >= 0.f && ny <= hy && nz >= 0.f && nz <= hz;
      const int lin = in ? ((int)nz * dy + (int)ny) * dx + (int)nx : 0;   // voxel 0: every volume has one
      const int d = dist2[lin];
      // rule 4
      const int c = (in && d >= 0) ? min(d, cap2) : cap2;
      cost += c;
      inliers += (in && d >= 0 && d <= inlier2) ? 1 : 0;
      outside += in ? 0 : 1;
    }
  }
  if (live) {                                       // rule 5: integer sums, any order
    atomicAdd(out + b * 3 + 0, (unsigned long long)cost);
    atomicAdd(out + b * 3 + 1, (unsigned long long)inliers);
    atomicAdd(out + b * 3 + 2, (unsigned long long)outside);
  }
}

}  // namespace

SGNN_EXPORT int sgnn_register_score(const float *points, int npoints, const int32_t *dist2, int dx, int dy, int dz,
                                    const sgnn_register_pose *poses, int nposes, int cap2, int inlier2, int64_t *out,
                                    sgnn_stream_t stream) {
  SGNN_CHECK_ARG(npoints >= 0 && nposes >= 0 && nposes <= SGNN_REGISTER_SCORE_MAX_POSES);
  SGNN_CHECK_ARG((int64_t)npoints < ((int64_t)1 << 31) - 65536);                                  // the tile count is an int
  SGNN_CHECK_ARG(dx >= 1 && dy >= 1 && dz >= 1 && (int64_t)dx * dy * dz < ((int64_t)1 << 31));   // the voxel is an int32
  SGNN_CHECK_ARG(cap2 > 0 && inlier2 >= 0);
  if (nposes == 0) return SGNN_OK;
  SGNN_CHECK_ARG(dist2 && poses && out && (points || npoints == 0));
  hipStream_t s = (hipStream_t)stream;
  SGNN_HIP_TRY(hipMemsetAsync(out, 0, (size_t)nposes * 3 * sizeof(int64_t), s));
  if (npoints == 0) return SGNN_OK;
  const int nblk = (nposes + BLOCK - 1) / BLOCK, ntiles = (npoints + TILE - 1) / TILE;
  const int slices = max(1, min(ntiles, min(65535, (TARGET_BLOCKS + nblk - 1) / nblk)));
  SGNN_LAUNCH(k_register_score, dim3(nblk, slices), dim3(BLOCK), 0, s, points, npoints, dist2, dx, dy, dz, poses, nposes,
              cap2, inlier2, (unsigned long long *)out);
  SGNN_CHECK_LAUNCH();
  return SGNN_OK;
}
