// The point-triangle routine of INTEGRATION.md section G, rule 2, shared by meshdist.hip (nearest triangle of arbitrary
// points) and voxelize.hip (the same for voxel centres, section L).  Both are built with -ffp-contract=off: every product
// and sum is rounded on its own and the divisions are correctly rounded, so the two agree bit for bit.
#pragma once
#include <math.h>
#include "common.h"

struct V3 {
  float x, y, z;
};

__device__ __forceinline__ V3 sub(const V3 &a, const V3 &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(const V3 &a, const V3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// a - s * b
__device__ __forceinline__ V3 away(const V3 &a, float s, const V3 &b) {
  return {a.x - s * b.x, a.y - s * b.y, a.z - s * b.z};
}
__device__ __forceinline__ bool finite3(const V3 &a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

// the closest feature of a triangle: which branch of rule 2 produced the residual (section L, rule 4)
enum TriFeature { TRI_VERT_A = 0, TRI_VERT_B, TRI_VERT_C, TRI_EDGE_AB, TRI_EDGE_AC, TRI_EDGE_BC, TRI_INTERIOR };

// rule 2: the residual e from the closest point of the triangle (a, a + ab, a + ac) to p, and the branch that gave it
__device__ __forceinline__ V3 tri_residual(const V3 &p, const V3 &a, const V3 &ab, const V3 &ac, int &feature) {
  const V3 ap = sub(p, a);
  const float d1 = dot(ab, ap), d2 = dot(ac, ap);
  V3 e;
  if (d1 <= 0.f && d2 <= 0.f) {
    e = ap;                                                       // vertex a
    feature = TRI_VERT_A;
  } else {
    const V3 bp = sub(ap, ab);
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.f && d4 <= d3) {
      e = bp;                                                     // vertex b
      feature = TRI_VERT_B;
    } else {
      const float vc = d1 * d4 - d3 * d2;
      if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
        e = away(ap, __fdiv_rn(d1, d1 - d3), ab);                 // edge ab
        feature = TRI_EDGE_AB;
      } else {
        const V3 cp = sub(ap, ac);
        const float d5 = dot(ab, cp), d6 = dot(ac, cp);
        if (d6 >= 0.f && d5 <= d6) {
          e = cp;                                                 // vertex c
          feature = TRI_VERT_C;
        } else {
          const float vb = d5 * d2 - d1 * d6;
          if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
            e = away(ap, __fdiv_rn(d2, d2 - d6), ac);             // edge ac
            feature = TRI_EDGE_AC;
          } else {
            const float va = d3 * d6 - d5 * d4;
            const float s = d4 - d3, t = d5 - d6;
            if (va <= 0.f && s >= 0.f && t >= 0.f) {
              e = away(bp, __fdiv_rn(s, s + t), sub(ac, ab));     // edge bc
              feature = TRI_EDGE_BC;
            } else {
              // interior.  v and w come from differences of nearly equal products; one refinement step on the
              // in-plane residual of e brings a thin triangle's result down to the rounding of its coordinates
              const float den = (va + vb) + vc;
              e = away(away(ap, __fdiv_rn(vb, den), ab), __fdiv_rn(vc, den), ac);
              const float r1 = dot(ab, e), r2 = dot(ac, e);
              const float g11 = dot(ab, ab), g12 = dot(ab, ac), g22 = dot(ac, ac);
              e = away(away(e, __fdiv_rn(r1 * g22 - r2 * g12, den), ab), __fdiv_rn(r2 * g11 - r1 * g12, den), ac);
              feature = TRI_INTERIOR;
            }
          }
        }
      }
    }
  }
  return e;
}

// rule 2: squared distance from p to the triangle (a, a + ab, a + ac)
__device__ __forceinline__ float tri_dist2(const V3 &p, const V3 &a, const V3 &ab, const V3 &ac) {
  int feature;
  const V3 e = tri_residual(p, a, ab, ac, feature);
  return (e.x * e.x + e.y * e.y) + e.z * e.z;
}
