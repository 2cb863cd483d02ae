// mi355r — What the point-to-triangle translation units (mr_pointmesh.hip, mr_icpmesh.hip) share: the triangle record,
// the pair function, the record's staged form (7 float4) and the compare loop of a staged chunk against the queries a
// thread keeps in registers.
//
//   tri_make / seg_dist / pair_dist   the pair function, float32 in one fixed operation order, no FMA, IEEE division
//                   and sqrtf. tri_make computes once per triangle what pair_dist reuses across queries (edge vectors
//                   and squared lengths, the unit normal, the barycentric terms, the plane flag).
//   tri_load        a packed face -> its record (plane = -1 for a vertex id out of range).
//   tri_stage / tri_staged   the record as 7 float4 and back; every lane reads the same record (a broadcast).
//   tri_scan        a staged chunk against Q queries, strict comparison: the lowest index wins a tie.
//   tri_closest     the closest point and the distance function's gradient direction of a pair.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mr_common.h"

#define MPM_REC 7                        // float4 per staged triangle record
#define MPM_EPS 1e-8f                    // upstream's kEpsilon, compared in float32

namespace {

// A triangle with what pair_dist reuses across queries. plane: 1 the plane branch is open (area >= the
// threshold and |n| > 1e-8), 0 edges only, -1 not a triangle of the mesh (a vertex id out of range): skipped.
struct Tri {
  float v0[3], v1[3], v2[3];
  float e01[3], e12[3], e20[3];  // v1 - v0, v2 - v1, v0 - v2
  float n[3];                    // unit normal (zeros when plane != 1)
  float l01, l12, l20;           // squared edge lengths
  float d01, nn;                 // e01 . (v2 - v0), |e01 x (v2 - v0)|^2
  int plane;
};

MR_DEV float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

MR_DEV Tri tri_make(const float* a, const float* b, const float* c, float min_area) {
  Tri t;
  float w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    t.v0[k] = a[k];
    t.v1[k] = b[k];
    t.v2[k] = c[k];
    t.e01[k] = b[k] - a[k];
    t.e12[k] = c[k] - b[k];
    t.e20[k] = a[k] - c[k];
    w[k] = -t.e20[k];  // v2 - v0, exactly
  }
  t.l01 = dot3(t.e01, t.e01);
  t.l12 = dot3(t.e12, t.e12);
  t.l20 = dot3(t.e20, t.e20);
  t.d01 = dot3(t.e01, w);
  float n[3];
  n[0] = t.e01[1] * w[2] - t.e01[2] * w[1];
  n[1] = t.e01[2] * w[0] - t.e01[0] * w[2];
  n[2] = t.e01[0] * w[1] - t.e01[1] * w[0];
  t.nn = dot3(n, n);
  const float len = sqrtf(t.nn);
  t.plane = (0.5f * len >= min_area && len > MPM_EPS) ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) t.n[k] = t.plane ? n[k] / len : 0.0f;
  return t;
}

// Squared distance of p to the segment a -> b (ab = b - a, l2 = ab . ab); t: the closest point is a + t ab.
// A segment with l2 <= 1e-8 is the point b.
MR_DEV float seg_dist(const float* p, const float* a, const float* b, const float* ab, float l2, float& t) {
  float d[3];
  if (l2 <= MPM_EPS) {
    t = 1.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = p[k] - b[k];
    return dot3(d, d);
  }
  float pa[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) pa[k] = p[k] - a[k];
  t = smin(smax(dot3(pa, ab) / l2, 0.0f), 1.0f);
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = p[k] - (a[k] + t * ab[k]);
  return dot3(d, d);
}

// d(p, tri). BARY: also the closest point's barycentrics bw[3], and in `inside` whether the plane branch returned the
// distance. The barycentrics of p's projection onto the plane are those of p itself over (e01, v2 - v0), the normal
// component of p - v0 being orthogonal to both; the denominator is |n|^2 (Lagrange's identity), which is > 1e-16
// whenever the plane branch is open.
template <bool BARY> MR_DEV float pair_dist(const float* p, const Tri& t, float* bw, bool* inside = nullptr) {
  if (BARY && inside) *inside = false;
  if (t.plane > 0) {
    float q[3], w[3], r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      q[k] = p[k] - t.v0[k];
      w[k] = -t.e20[k];
      r[k] = t.v0[k] - p[k];
    }
    const float d20 = dot3(q, t.e01), d21 = dot3(q, w);
    const float b1 = (t.l20 * d20 - t.d01 * d21) / t.nn;
    const float b2 = (t.l01 * d21 - t.d01 * d20) / t.nn;
    const float b0 = (1.0f - b1) - b2;
    if (b0 >= 0.0f && b0 <= 1.0f && b1 >= 0.0f && b1 <= 1.0f && b2 >= 0.0f && b2 <= 1.0f) {
      const float h = dot3(r, t.n);
      if (BARY) {
        bw[0] = b0;
        bw[1] = b1;
        bw[2] = b2;
        if (inside) *inside = true;
      }
      return h * h;
    }
  }
  float t0, t1, t2;
  const float s0 = seg_dist(p, t.v0, t.v1, t.e01, t.l01, t0);
  const float s1 = seg_dist(p, t.v1, t.v2, t.e12, t.l12, t1);
  const float s2 = seg_dist(p, t.v2, t.v0, t.e20, t.l20, t2);
  float best = s0;
  int e = 0;
  if (s1 < best) {
    best = s1;
    e = 1;
  }
  if (s2 < best) {
    best = s2;
    e = 2;
  }
  if (BARY) {
    const float tt = e == 0 ? t0 : (e == 1 ? t1 : t2);
    bw[0] = e == 0 ? 1.0f - tt : (e == 2 ? tt : 0.0f);  // (1 - t, t) on the edge's two ends, 0 opposite
    bw[1] = e == 1 ? 1.0f - tt : (e == 0 ? tt : 0.0f);
    bw[2] = e == 2 ? 1.0f - tt : (e == 1 ? tt : 0.0f);
  }
  return best;
}

// The pair's distance, its closest point q = (b0 v0 + b1 v1) + b2 v2 and the unit gradient direction n of the
// distance function at p: the record's normal where the plane branch returned the distance, else (p - q) / |p - q|
// (zeros when |p - q| <= 1e-8). On an edge or vertex shared by several faces n does not depend on which of them won.
MR_DEV float tri_closest(const float* p, const Tri& t, float* q, float* n) {
  float bw[3];
  bool inside;
  const float d = pair_dist<true>(p, t, bw, &inside);
  float e[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    q[k] = (bw[0] * t.v0[k] + bw[1] * t.v1[k]) + bw[2] * t.v2[k];
    e[k] = p[k] - q[k];
  }
  const float l = sqrtf(dot3(e, e));
#pragma unroll
  for (int k = 0; k < 3; ++k) n[k] = inside ? t.n[k] : (l > MPM_EPS ? e[k] / l : 0.0f);
  return d;
}

// Mesh n's range of a packed array of `total` elements; a range that does not lie inside it counts as empty.
MR_DEV void range_of(const int64_t* __restrict__ first, const int64_t* __restrict__ count, int64_t n, int64_t total,
                     int64_t& f, int64_t& c) {
  f = first[n];
  c = count[n];
  if (f < 0 || c <= 0 || f > total || c > total - f || c >= 0x7fffffffll) {
    f = 0;
    c = 0;
  }
}

// Packed face f of `faces` over the V vertices of `verts`, with its vertex ids; plane = -1 when an id lies outside
// the vertices.
MR_DEV Tri tri_load(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, float min_area,
                    int64_t f, int& ia, int& ib, int& ic) {
  ia = faces[3 * f];
  ib = faces[3 * f + 1];
  ic = faces[3 * f + 2];
  if (ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V) {
    Tri t = {};
    t.plane = -1;
    return t;
  }
  return tri_make(verts + 3 * (int64_t)ia, verts + 3 * (int64_t)ib, verts + 3 * (int64_t)ic, min_area);
}

MR_DEV void tri_stage(float4* __restrict__ r, const Tri& t) {
  r[0] = make_float4(t.v0[0], t.v0[1], t.v0[2], t.l01);
  r[1] = make_float4(t.v1[0], t.v1[1], t.v1[2], t.l12);
  r[2] = make_float4(t.v2[0], t.v2[1], t.v2[2], t.l20);
  r[3] = make_float4(t.e01[0], t.e01[1], t.e01[2], t.d01);
  r[4] = make_float4(t.e12[0], t.e12[1], t.e12[2], t.nn);
  r[5] = make_float4(t.e20[0], t.e20[1], t.e20[2], __int_as_float(t.plane));
  r[6] = make_float4(t.n[0], t.n[1], t.n[2], 0.0f);
}

// UNIFORM: every lane reads the same record, so the plane flag is a scalar.
template <bool UNIFORM = true> MR_DEV Tri tri_staged(const float4* __restrict__ r) {
  const float4 a = r[0], b = r[1], c = r[2], d = r[3], e = r[4], f = r[5], g = r[6];
  Tri t;
  t.v0[0] = a.x; t.v0[1] = a.y; t.v0[2] = a.z; t.l01 = a.w;
  t.v1[0] = b.x; t.v1[1] = b.y; t.v1[2] = b.z; t.l12 = b.w;
  t.v2[0] = c.x; t.v2[1] = c.y; t.v2[2] = c.z; t.l20 = c.w;
  t.e01[0] = d.x; t.e01[1] = d.y; t.e01[2] = d.z; t.d01 = d.w;
  t.e12[0] = e.x; t.e12[1] = e.y; t.e12[2] = e.z; t.nn = e.w;
  t.e20[0] = f.x; t.e20[1] = f.y; t.e20[2] = f.z;
  t.plane = UNIFORM ? __builtin_amdgcn_readfirstlane(__float_as_int(f.w)) : __float_as_int(f.w);
  t.n[0] = g.x; t.n[1] = g.y; t.n[2] = g.z;
  return t;
}

// The cnt records staged in sm against the Q queries p: best / bi keep the smallest distance and its place in the
// chunk. The comparison is strict: the lowest index wins a tie inside the chunk.
template <int Q>
MR_DEV void tri_scan(const float4* __restrict__ sm, int cnt, const float (&p)[Q][3], float (&best)[Q], int (&bi)[Q]) {
  for (int j = 0; j < cnt; ++j) {
    const Tri t = tri_staged(sm + MPM_REC * j);
    if (t.plane < 0) continue;  // wave-uniform
#pragma unroll
    for (int k = 0; k < Q; ++k) {
      const float dd = pair_dist<false>(p[k], t, nullptr);
      if (dd < best[k]) {
        best[k] = dd;
        bi[k] = j;
      }
    }
  }
}

}  // namespace
