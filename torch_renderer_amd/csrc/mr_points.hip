// mi355r — point-cloud losses and mesh sampling (PyTorch3D chamfer_distance with K = 1 nearest neighbours,
// sample_points_from_meshes' point construction, face areas): mr_nearest_points / mr_chamfer_* /
// mr_sample_points_* / mr_face_areas of include/mi355r.h. A translation unit of its own (the render kernels of
// mr_raster.hip and the priors of mr_priors.hip are compiled as before).
//
//   k_nn            both directions (x -> y, y -> x) of a batch in one launch, over the scan of mr_cloud.h: a
//                   workgroup takes 512 queries (4 per thread) and one chunk of <= 1024 targets (one LDS read feeds 4
//                   distance evaluations, 44 VALU instructions: the loop is VALU-bound). The target
//                   range is split into chunks over workgroups (the host picks the chunk so that ~1024 workgroups
//                   exist per direction); each thread merges its chunk's minimum into the key buffer (nn_key, set to
//                   all-ones by a memset ahead of the launch) with a 64-bit atomicMin.
//                   dist = (dx*dx + dy*dy) + dz*dz or (|dx| + |dy|) + |dz| in float32, no FMA.
//   k_nn_reduce     keys -> dist (float32) / idx (int32) per point, 0 / -1 for entries past a length or of a cloud
//                   whose counterpart is empty; per-workgroup partial sums of dist (double, fixed tree).
//   k_cham_final    per cloud: sums the partials in order, applies weights and the point reduction; then the batch
//                   reduction in a fixed order. Also leaves the backward's per-cloud coefficients.
//   k_cham_scatter  backward, the many-to-one part: every query adds (q - t) (norm 2) or sign(q - t) (norm 1) to its
//                   target's row with 64-bit fixed-point integer atomics (mr_common.h; addends >= MR_FIX_MAX go to
//                   a float remainder row). The rows hold UNSCALED differences: the coefficients are applied after.
//   k_cham_grad     backward: grad = k (c_own (p - nn(p)) - c_other row(p)), k = 2 or 1, one store per entry.
//   k_sample_fwd / k_sample_scatter / k_fix_to_float, k_face_areas: see the entry points below.
//   k_icp_*         iterative_closest_point and corresponding_points_alignment (mr_icp_* / mr_points_alignment). An
//                   ICP iteration is four launches and no host work: k_icp_nn (k_nn's x -> y direction with the
//                   cloud's transform applied in registers), k_icp_moments (float64 sums of y_nn and (x - mx) y_nn^T
//                   per tile), k_icp_solve (every workgroup of a cloud sums the tiles in order and solves the 3x3
//                   Procrustes problem by a fixed-sweep Jacobi SVD in float64, then sums its tile of the residual
//                   under the new transform) and k_icp_status (rmse, relative drop, the device status words every
//                   kernel of a later iteration reads first). No float atomics, every sum in a fixed order.
//                   mr_icp_iterate_grid / mr_icp_plane_iterate_grid put k_icp_nn_grid in k_icp_nn's place: the same
//                   key per source point from a walk through a point grid of the targets (mr_grid.h's grid_walk).
//   k_icp_plane_*   the point-to-plane estimator on the same loop (mr_icp_plane_iterate): k_icp_nn as it is, then
//                   k_icp_plane_moments (validity, float64 sums of J J^T, J r and the pair count per tile),
//                   k_icp_plane_solve (a damped 6x6 Cholesky step about the transformed source mean, then the new
//                   residual) and k_icp_plane_status (the pair count as divisor). The step, the last two kernels, the
//                   loop's workspace and the status rule live in mr_icp.h, which mr_icpmesh.hip shares.
//   k_posed_*     the chamfer distance of ONE cloud pair under S poses (mr_posed_chamfer): k_posed_nn, a workgroup
//                   per (pose, direction, 512 queries) that scans all targets itself, and k_posed_final (see there).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mi355r.h"
#include "mr_common.h"
#include "mr_host.h"
#include "mr_cloud.h"
#include "mr_grid.h"
#include "mr_icp.h"

#define MRN_Q 4                        // queries per thread
#define MRN_QT (MRN_BLOCK * MRN_Q)     // queries per workgroup
#define MRN_MINCHUNK 64                // targets staged per workgroup at least (at most MRN_MAXCHUNK)
#define MRN_WANT_GROUPS 1024           // workgroups per direction the chunk size aims for

namespace {

struct NNGeom {
  int64_t N, P[2];     // clouds; points of x and of y (padded)
  int chunk[2];        // targets per workgroup of direction d (d = 0: queries x, targets y)
  int64_t nchunk[2];   // chunks of direction d
  int64_t groups[2];   // workgroups of direction d per cloud
};

NNGeom nn_geom(int64_t N, int64_t P1, int64_t P2, int64_t want_groups = MRN_WANT_GROUPS) {
  NNGeom g;
  g.N = N;
  g.P[0] = P1;
  g.P[1] = P2;
  for (int d = 0; d < 2; ++d) {
    const int64_t Pq = g.P[d], Pt = g.P[1 - d];
    const int64_t qtiles = ceil_div(Pq, MRN_QT);
    int64_t want = want_groups / (N * qtiles);
    if (want < 1) want = 1;
    int64_t c = ((Pt + want - 1) / want + 63) / 64 * 64;
    if (c < MRN_MINCHUNK) c = MRN_MINCHUNK;
    if (c > MRN_MAXCHUNK) c = MRN_MAXCHUNK;
    g.chunk[d] = (int)c;
    g.nchunk[d] = (Pt + c - 1) / c;
    g.groups[d] = qtiles * g.nchunk[d];
  }
  return g;
}

struct PointsWS {
  u64* key[2];    // (N, P1), (N, P2)
  double* part;   // (2, N, nblk)
  int64_t nblk;
  size_t key_bytes, bytes;
};
PointsWS carve_points(void* base, int64_t N, int64_t P1, int64_t P2) {
  PointsWS w;
  Carver c(base);
  w.key[0] = c.take_packed<u64>((size_t)(N * P1));  // the two key arrays back to back: one memset
  w.key[1] = c.take<u64>((size_t)(N * P2));
  w.key_bytes = sizeof(u64) * (size_t)(N * (P1 + P2));
  w.nblk = ceil_div(P1 > P2 ? P1 : P2, MRR_TILE);
  w.part = c.take<double>(2 * (size_t)(N * w.nblk));
  w.bytes = c.off;
  return w;
}

// A workgroup's share of a chunked search: workgroup `group` of a cloud takes query tile group / nchunk and target
// chunk group % nchunk, and merges each query's nearest target of the chunk into key[query].
template <int NORM>
__device__ __forceinline__ void nn_chunk_search(float4* __restrict__ sm, const float* __restrict__ q,
                                                const float* __restrict__ t, int64_t lq, int64_t lt, int64_t group,
                                                int64_t nchunk, int chunk, const float* __restrict__ tr, bool apply,
                                                u64* __restrict__ key) {
  const int64_t q0 = (group / nchunk) * MRN_QT;
  const int64_t t0 = (group % nchunk) * chunk;
  if (q0 >= lq || t0 >= lt) return;  // uniform over the workgroup
  const int cnt = (int)((lt - t0 < chunk) ? lt - t0 : chunk);
  scan_stage(sm, t, t0, cnt, nullptr, false);
  __syncthreads();

  float qx[MRN_Q], qy[MRN_Q], qz[MRN_Q], best[MRN_Q];
  int bi[MRN_Q];
  scan_load_queries(q, q0, lq, tr, apply, qx, qy, qz);
#pragma unroll
  for (int k = 0; k < MRN_Q; ++k) {
    best[k] = __builtin_inff();
    bi[k] = 0;
  }
  scan_nearest<NORM>(sm, cnt, 0, qx, qy, qz, best, bi);
#pragma unroll
  for (int k = 0; k < MRN_Q; ++k) {
    const int64_t i = q0 + k * MRN_BLOCK + threadIdx.x;
    if (i < lq) atomicMin(&key[i], nn_key(best[k], (uint32_t)(t0 + bi[k])));
  }
}

template <int NORM>
__global__ void __launch_bounds__(MRN_BLOCK) k_nn(const float* __restrict__ x, const float* __restrict__ y, NNGeom g,
                                                  const int64_t* __restrict__ xl, const int64_t* __restrict__ yl,
                                                  u64* __restrict__ key_x, u64* __restrict__ key_y) {
  __shared__ float4 sm[MRN_MAXCHUNK];
  const int d = blockIdx.z;
  if ((int64_t)blockIdx.x >= g.groups[d]) return;
  const int64_t n = blockIdx.y;
  const int64_t Pq = g.P[d], Pt = g.P[1 - d];
  nn_chunk_search<NORM>(sm, (d ? y : x) + 3 * n * Pq, (d ? x : y) + 3 * n * Pt, cloud_len(d ? yl : xl, n, Pq),
                        cloud_len(d ? xl : yl, n, Pt), blockIdx.x, g.nchunk[d], g.chunk[d], nullptr, false,
                        (d ? key_y : key_x) + n * Pq);
}

// grid (nblk, N, directions). dist / idx / part may each be NULL.
__global__ void __launch_bounds__(MRR_BLOCK) k_nn_reduce(NNGeom g, const int64_t* __restrict__ xl,
                                                         const int64_t* __restrict__ yl, const u64* __restrict__ key_x,
                                                         const u64* __restrict__ key_y, float* __restrict__ dist_x,
                                                         int32_t* __restrict__ idx_x, float* __restrict__ dist_y,
                                                         int32_t* __restrict__ idx_y, double* __restrict__ part,
                                                         int64_t nblk) {
  __shared__ double sm[4];
  const int d = blockIdx.z;
  const int64_t n = blockIdx.y;
  const int64_t Pq = g.P[d], Pt = g.P[1 - d];
  const int64_t lq = cloud_len(d ? yl : xl, n, Pq), lt = cloud_len(d ? xl : yl, n, Pt);
  const u64* __restrict__ key = (d ? key_y : key_x) + n * Pq;
  float* __restrict__ dist = d ? dist_y : dist_x;
  int32_t* __restrict__ idx = d ? idx_y : idx_x;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < MRR_PER; ++k) {
    const int64_t i = (int64_t)blockIdx.x * MRR_TILE + k * MRR_BLOCK + threadIdx.x;
    if (i >= Pq) continue;
    const bool ok = i < lq && lt > 0;
    const u64 kk = ok ? key[i] : 0;
    const float dv = ok ? key_dist(kk) : 0.0f;
    if (dist) dist[n * Pq + i] = dv;
    if (idx) idx[n * Pq + i] = ok ? (int32_t)key_index(kk) : -1;
    s += (double)dv;
  }
  if (part) {  // uniform
    s = block_sum(s, sm);
    if (threadIdx.x == 0) part[((int64_t)d * g.N + n) * nblk + blockIdx.x] = s;
  }
}

// One workgroup. Thread t takes clouds t, t + 256, ...: each cloud's partials are summed in order; out[n] for
// batch_reduction None, else the clouds' values are summed per thread in order and then in the fixed tree.
// coef (2, N): d loss / d (cloud n's point sum of direction d) for an upstream gradient of 1.
__global__ void __launch_bounds__(MRR_BLOCK) k_cham_final(const double* __restrict__ part, int64_t nblk, int64_t N,
                                                          int64_t P1, int64_t P2, const int64_t* __restrict__ xl,
                                                          const int64_t* __restrict__ yl,
                                                          const float* __restrict__ weights, int flags,
                                                          float* __restrict__ out, float* __restrict__ coef) {
  __shared__ double sm[4];
  const bool single = flags & MR_CHAMFER_SINGLE, pmean = flags & MR_CHAMFER_POINT_MEAN;
  double wsum = 0.0;
  for (int64_t n = threadIdx.x; n < N; n += MRR_BLOCK) wsum += weights ? (double)weights[n] : 1.0;
  wsum = block_sum(wsum, sm);
  double scale = 1.0;  // of the batch reduction
  if (flags & MR_CHAMFER_BATCH_MEAN) {
    const double div = weights ? wsum : (double)(N > 1 ? N : 1);
    scale = div != 0.0 ? 1.0 / div : 0.0;
  }
  const bool per_cloud = !(flags & (MR_CHAMFER_BATCH_MEAN | MR_CHAMFER_BATCH_SUM));
  double total = 0.0;
  for (int64_t n = threadIdx.x; n < N; n += MRR_BLOCK) {
    const int64_t lx = cloud_len(xl, n, P1), ly = cloud_len(yl, n, P2);
    const double w = weights ? (double)weights[n] : 1.0;
    double v = 0.0;
    for (int d = 0; d < (single ? 1 : 2); ++d) {
      const int64_t lq = d ? ly : lx, lt = d ? lx : ly;
      const double c = w * (pmean ? 1.0 / (double)(lq > 1 ? lq : 1) : 1.0);
      double s = 0.0;
      for (int64_t b = 0; b < nblk; ++b) s += part[((int64_t)d * N + n) * nblk + b];
      v += c * s;
      if (coef) coef[(int64_t)d * N + n] = lt > 0 ? (float)(c * scale) : 0.0f;
    }
    if (single && coef) coef[N + n] = 0.0f;
    if (per_cloud) out[n] = (float)v;
    total += v;
  }
  total = block_sum(total, sm);
  if (!per_cloud && threadIdx.x == 0) out[0] = (float)(total * scale);
}

// grid (blocks over max(P1, P2), N, directions): point i of direction d's queries adds its difference to its
// target's row. fix / rem: (N, P1, 3) rows of x then (N, P2, 3) rows of y.
template <int NORM>
__global__ void __launch_bounds__(MRR_BLOCK) k_cham_scatter(const float* __restrict__ x, const float* __restrict__ y,
                                                            int64_t N, int64_t P1, int64_t P2,
                                                            const int32_t* __restrict__ idx_x,
                                                            const int32_t* __restrict__ idx_y, u64* __restrict__ fix,
                                                            float* __restrict__ rem) {
  const int d = blockIdx.z;
  const int64_t n = blockIdx.y;
  const int64_t Pq = d ? P2 : P1, Pt = d ? P1 : P2;
  const int64_t i = (int64_t)blockIdx.x * MRR_BLOCK + threadIdx.x;
  if (i >= Pq) return;
  const int32_t j = (d ? idx_y : idx_x)[n * Pq + i];
  if (j < 0 || j >= Pt) return;
  const float* __restrict__ q = (d ? y : x) + 3 * (n * Pq + i);
  const float* __restrict__ t = (d ? x : y) + 3 * (n * Pt + j);
  const int64_t row = 3 * ((d ? 0 : N * P1) + n * Pt + j);  // the target's row
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float df = q[c] - t[c];
    fix_add(fix, rem, row + c, NORM == 2 ? df : sgn(df));
  }
}

template <int NORM>
__global__ void __launch_bounds__(MRR_BLOCK) k_cham_grad(const float* __restrict__ x, const float* __restrict__ y,
                                                         int64_t N, int64_t P1, int64_t P2,
                                                         const int32_t* __restrict__ idx_x,
                                                         const int32_t* __restrict__ idx_y,
                                                         const float* __restrict__ coef, const float* __restrict__ g,
                                                         int g_per_cloud, const u64* __restrict__ fix,
                                                         const float* __restrict__ rem, float* __restrict__ grad_x,
                                                         float* __restrict__ grad_y) {
  const int d = blockIdx.z;
  const int64_t n = blockIdx.y;
  const int64_t Pq = d ? P2 : P1, Pt = d ? P1 : P2;
  const int64_t i = (int64_t)blockIdx.x * MRR_BLOCK + threadIdx.x;
  if (i >= Pq) return;
  const float up = g_per_cloud ? g[n] : g[0];
  const float k = NORM == 2 ? 2.0f : 1.0f;
  const float c_own = k * up * coef[(int64_t)d * N + n], c_other = k * up * coef[(int64_t)(1 - d) * N + n];
  const int32_t* __restrict__ idx = d ? idx_y : idx_x;
  const int32_t j = idx ? idx[n * Pq + i] : -1;
  const bool has = j >= 0 && j < Pt;
  const float* __restrict__ q = (d ? y : x) + 3 * (n * Pq + i);
  const float* __restrict__ t = (d ? x : y) + 3 * (n * Pt + (has ? j : 0));
  const int64_t row = 3 * ((d ? N * P1 : 0) + n * Pq + i);  // this point's own row
  float* __restrict__ out = (d ? grad_y : grad_x) + 3 * (n * Pq + i);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float own = 0.0f;
    if (has) {
      const float df = q[c] - t[c];
      own = NORM == 2 ? df : sgn(df);
    }
    const float other = fix_read(fix, rem, row + c);
    out[c] = c_own * own - c_other * other;
  }
}

__device__ __forceinline__ bool face_ok(const int32_t* __restrict__ faces, int64_t F, int64_t V, int64_t f, int& a,
                                        int& b, int& c) {
  if (f < 0 || f >= F) return false;
  a = faces[3 * f];
  b = faces[3 * f + 1];
  c = faces[3 * f + 2];
  return a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V;
}

__device__ __forceinline__ void bary_of(float u, float v, float& w0, float& w1, float& w2) {
  const float s = sqrtf(u);
  w0 = 1.0f - s;
  w1 = s * (1.0f - v);
  w2 = s * v;
}

// Sample m (of M = N * S): p = (w0 a + w1 b) + w2 c of face face_idx[m]; zeros for a negative (or out-of-range) id.
__global__ void __launch_bounds__(MRR_BLOCK) k_sample_fwd(const float* __restrict__ verts, int64_t V,
                                                          const int32_t* __restrict__ faces, int64_t F,
                                                          const int32_t* __restrict__ face_idx,
                                                          const float* __restrict__ uv, int64_t M,
                                                          float* __restrict__ out) {
  const int64_t m = (int64_t)blockIdx.x * MRR_BLOCK + threadIdx.x;
  if (m >= M) return;
  int a, b, c;
  float p[3] = {0.0f, 0.0f, 0.0f};
  if (face_ok(faces, F, V, face_idx[m], a, b, c)) {
    float w0, w1, w2;
    bary_of(uv[m], uv[M + m], w0, w1, w2);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = (w0 * verts[3 * (int64_t)a + k] + w1 * verts[3 * (int64_t)b + k]) + w2 * verts[3 * (int64_t)c + k];
  }
  out[3 * m] = p[0];
  out[3 * m + 1] = p[1];
  out[3 * m + 2] = p[2];
}

__global__ void __launch_bounds__(MRR_BLOCK) k_sample_scatter(int64_t V, const int32_t* __restrict__ faces, int64_t F,
                                                              const int32_t* __restrict__ face_idx,
                                                              const float* __restrict__ uv, int64_t M,
                                                              const float* __restrict__ gp, u64* __restrict__ fix,
                                                              float* __restrict__ rem) {
  const int64_t m = (int64_t)blockIdx.x * MRR_BLOCK + threadIdx.x;
  if (m >= M) return;
  int a, b, c;
  if (!face_ok(faces, F, V, face_idx[m], a, b, c)) return;
  float w0, w1, w2;
  bary_of(uv[m], uv[M + m], w0, w1, w2);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float gk = gp[3 * m + k];
    fix_add(fix, rem, 3 * (int64_t)a + k, w0 * gk);
    fix_add(fix, rem, 3 * (int64_t)b + k, w1 * gk);
    fix_add(fix, rem, 3 * (int64_t)c + k, w2 * gk);
  }
}

__global__ void __launch_bounds__(MRR_BLOCK) k_fix_to_float(const u64* __restrict__ fix, const float* __restrict__ rem,
                                                            int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * MRR_BLOCK + threadIdx.x;
  if (i < n) out[i] = fix_read(fix, rem, i);
}

__global__ void __launch_bounds__(MRR_BLOCK) k_face_areas(const float* __restrict__ verts, int64_t V,
                                                          const int32_t* __restrict__ faces, int64_t F,
                                                          float* __restrict__ areas) {
  const int64_t f = (int64_t)blockIdx.x * MRR_BLOCK + threadIdx.x;
  if (f >= F) return;
  int a, b, c;
  float area = 0.0f;
  if (face_ok(faces, F, V, f, a, b, c)) {
    const float* pa = verts + 3 * (int64_t)a;
    const float* pb = verts + 3 * (int64_t)b;
    const float* pc = verts + 3 * (int64_t)c;
    const float ux = pb[0] - pa[0], uy = pb[1] - pa[1], uz = pb[2] - pa[2];
    const float vx = pc[0] - pa[0], vy = pc[1] - pa[1], vz = pc[2] - pa[2];
    const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    area = 0.5f * sqrtf((cx * cx + cy * cy) + cz * cz);
  }
  areas[f] = area;
}

int check_clouds(const char* who, const float* x, const float* y, int64_t N, int64_t P1, int64_t P2, int32_t norm) {
  if (int rc = check_sizes(who, N, P1, P2)) return rc;
  if (norm != 1 && norm != 2) return set_err(MR_EINVAL, "%s: norm must be 1 or 2", who);
  if (!x || !y) return set_err(MR_EINVAL, "%s: x / y is NULL", who);
  return MR_OK;
}

// memset of the keys + k_nn for `dirs` directions.
int run_nn(const float* x, const float* y, const NNGeom& g, const int64_t* xl, const int64_t* yl, int32_t norm, int dirs,
           const PointsWS& w, hipStream_t st) {
  if (g.groups[0] > 0x7fffffffll || g.groups[1] > 0x7fffffffll)
    return set_err(MR_EUNSUPPORTED, "nearest points: P1 * P2 is too large for one launch");
  if (int rc = memset_async(w.key[0], 0xff, w.key_bytes, st)) return rc;
  const int64_t gx = (dirs == 2 && g.groups[1] > g.groups[0]) ? g.groups[1] : g.groups[0];
  const dim3 grid((unsigned)gx, (unsigned)g.N, (unsigned)dirs);
  return launch(KID_NONE, "k_nn", norm == 2 ? k_nn<2> : k_nn<1>, grid, MRN_BLOCK, 0, st, x, y, g, xl, yl, w.key[0], w.key[1]);
}

bool mesh_sizes_ok(int64_t V, int64_t F, int64_t M) {
  return V >= 0 && F >= 0 && M >= 0 && V < 0x7fffffffll / 3 && F < 0x7fffffffll / 3 && M < (1ll << 31) * MRR_BLOCK / 4;
}

// ---------------------------------------------------------------------------
// Similarity alignment and ICP (PyTorch3D corresponding_points_alignment / iterative_closest_point).
// A cloud's transform is the 13 floats of sim_apply (mr_cloud.h).
// ---------------------------------------------------------------------------
// k_icp_nn workgroups the target chunk aims for. More than k_nn's: at the registration shape (300 clouds, 2,000
// sources, 100-400 targets) that is the minimum chunk of 64, whose many short workgroups even out the clouds'
// different target counts: 9.6 -> 7.9 ms per 97-iteration registration against 1,024 (ICP).
#ifndef MRI_WANT_GROUPS
#define MRI_WANT_GROUPS 16384
#endif
#define MRI_SWEEPS 10   // Jacobi sweeps of the 3x3 SVD (a converged pair is skipped; the count is fixed)

__device__ __forceinline__ float point_weight(const float* __restrict__ weights, int64_t n, int64_t P, int64_t i,
                                              int64_t len) {
  if (i >= len) return 0.0f;
  return weights ? weights[n * P + i] : 1.0f;
}

// One workgroup per cloud: its constants xc, and (rts != NULL) its starting transform (R0, T0, s0 or the identity).
__global__ void __launch_bounds__(MRR_BLOCK) k_icp_xstats(const float* __restrict__ x, int64_t P,
                                                          const int64_t* __restrict__ xl,
                                                          const float* __restrict__ weights, double eps,
                                                          double* __restrict__ xc, const float* __restrict__ R0,
                                                          const float* __restrict__ T0, const float* __restrict__ s0,
                                                          float* __restrict__ rts) {
  __shared__ double sm[4 * 4];
  const int64_t n = blockIdx.x;
  const int64_t len = cloud_len(xl, n, P);
  const float* __restrict__ q = x + 3 * n * P;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < len; i += MRR_BLOCK) {
    const double w = (double)point_weight(weights, n, P, i, len);
    a[0] += w;
    a[1] += w * (double)q[3 * i];
    a[2] += w * (double)q[3 * i + 1];
    a[3] += w * (double)q[3 * i + 2];
  }
  block_sums<MRR_BLOCK / 64>(a, sm);
  const double wc = a[0] > eps ? a[0] : eps;
  const double m0 = a[1] / wc, m1 = a[2] / wc, m2 = a[3] / wc;
  double b[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < len; i += MRR_BLOCK) {
    const double w = (double)point_weight(weights, n, P, i, len);
    const double d0 = (double)q[3 * i] - m0, d1 = (double)q[3 * i + 1] - m1, d2 = (double)q[3 * i + 2] - m2;
    b[0] += w * ((d0 * d0 + d1 * d1) + d2 * d2);
    b[1] += w * d0;
    b[2] += w * d1;
    b[3] += w * d2;
  }
  block_sums<MRR_BLOCK / 64>(b, sm);
  if (threadIdx.x == 0) {
    double* o = xc + n * MRI_XC;
    o[0] = a[0];
    o[1] = m0;
    o[2] = m1;
    o[3] = m2;
    o[4] = b[0];
    o[5] = b[1];
    o[6] = b[2];
    o[7] = b[3];
  }
  if (rts && threadIdx.x < MRI_RTS) {
    const int k = threadIdx.x;
    float v;
    if (k < 9) v = R0 ? R0[n * 9 + k] : ((k == 0 || k == 4 || k == 8) ? 1.0f : 0.0f);
    else if (k < 12) v = T0 ? T0[n * 3 + (k - 9)] : 0.0f;
    else v = s0 ? s0[n] : 1.0f;
    rts[n * MRI_RTS + k] = v;
  }
}

// k_nn's direction x -> y with the cloud's current transform applied to the queries in registers.
__global__ void __launch_bounds__(MRN_BLOCK) k_icp_nn(const float* __restrict__ x, const float* __restrict__ y, NNGeom g,
                                                      const int64_t* __restrict__ xl, const int64_t* __restrict__ yl,
                                                      const float* __restrict__ rts,
                                                      const int32_t* __restrict__ status, int max_iter,
                                                      u64* __restrict__ key_x) {
  __shared__ float4 sm[MRN_MAXCHUNK];
  if (icp_idle(status, max_iter)) return;
  if ((int64_t)blockIdx.x >= g.groups[0]) return;
  const int64_t n = blockIdx.y;
  const int64_t Pq = g.P[0], Pt = g.P[1];
  nn_chunk_search<2>(sm, x + 3 * n * Pq, y + 3 * n * Pt, cloud_len(xl, n, Pq), cloud_len(yl, n, Pt), blockIdx.x,
                     g.nchunk[0], g.chunk[0], rts + n * MRI_RTS, true, key_x + n * Pq);
}

// k_icp_nn through a point grid of the targets (mr_grid.hip builds it): grid (blocks over P1, N), one wave a workgroup,
// a source point per lane as in k_knn_grid; the lane transforms its point, walks the rings with a one-entry list and
// stores its key with a plain store (it owns the query). A cloud without targets stores nothing: the key stays
// all-ones, "no target" to the moments kernels.
//
// The key is k_icp_nn's, bit for bit. nn_chunk_search starts every chunk at (+inf, the chunk's first index) and lets a
// target in on a strictly smaller distance, and the chunks merge by atomicMin: the result is the smallest 64-bit key
// among nn_key(+inf, 0) and the keys of the targets whose distance is below +inf. So the list starts at
// nn_key(+inf, 0), not at k_knn_grid's all-ones, and a candidate enters on a strictly smaller 64-bit key
// (visit_range): a distance of +inf gives a key >= the start value, a nan's bits lie above +inf's, and neither
// displaces it; a query whose every distance is +inf or a nan ends with nn_key(+inf, 0) on both routes. Such a lane
// never stops early (inf < ring_bound is false), so it has seen every target when the rings cover the grid.
//
// CAP (the plane estimator with max_dist2 < +inf): the lane also stops after ring r >= 1 once ring_bound(r) >
// max_dist2. Every target beyond the rings then has a float32 distance >= the bound > max_dist2 and could not form a
// valid pair. If the lane's best is <= max_dist2 it lies strictly below every unvisited distance and is the nearest
// target; if it is above, so is the nearest target's, and k_icp_plane_moments writes idx = -1 for either key. Nothing
// downstream reads more of the key than that (DESIGN.md §3 "ICP through a point grid").
template <bool CAP>
__global__ void __launch_bounds__(MRG_QBLOCK) k_icp_nn_grid(const float* __restrict__ x, int64_t P1, int64_t P2,
                                                            const int64_t* __restrict__ xl,
                                                            const int64_t* __restrict__ yl, int64_t budget,
                                                            const GridHead* __restrict__ heads,
                                                            const uint32_t* __restrict__ cell_start,
                                                            const float4* __restrict__ pts,
                                                            const float* __restrict__ rts, float max_dist2,
                                                            const int32_t* __restrict__ status, int max_iter,
                                                            u64* __restrict__ key_x, u64* __restrict__ visited) {
  if (icp_idle(status, max_iter)) return;
  const int64_t n = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * MRG_QBLOCK + threadIdx.x;
  const int64_t lq = cloud_len(xl, n, P1);
  const uint32_t lt = (uint32_t)cloud_len(yl, n, P2);
  const GridHead H = heads[n];
  int gx, gy, gz;
  head_dims(H, budget, gx, gy, gz);
  uint32_t seen = 0u;
  if (i < lq && lt > 0u) {
    const float* __restrict__ q = x + 3 * (n * P1 + i);
    float qx, qy, qz;
    sim_apply(rts + n * MRI_RTS, q[0], q[1], q[2], qx, qy, qz);
    u64 L[1] = {nn_key(__builtin_inff(), 0u)};
    grid_walk<2, 1, CAP>(H, gx, gy, gz, cell_start + n * (budget + 1), pts + n * P2, lt, (uint32_t)(P2 - 1), qx, qy, qz,
                         1, max_dist2, L, seen);
    key_x[n * P1 + i] = L[0];
  }
  if (visited) grid_count_visited(seen, visited);
}

// grid (nblk, N): the moments of a tile of source points against their correspondences. key != NULL: the
// correspondence of point i is the index in key[i] (left in idx[i]; the key is set back to all-ones for the next
// search); key == NULL: point i of y.
__global__ void __launch_bounds__(MRR_BLOCK) k_icp_moments(const float* __restrict__ x, const float* __restrict__ y,
                                                           int64_t P1, int64_t P2, const int64_t* __restrict__ xl,
                                                           const int64_t* __restrict__ yl,
                                                           const float* __restrict__ weights,
                                                           const double* __restrict__ xc,
                                                           const int32_t* __restrict__ status, int max_iter,
                                                           u64* __restrict__ key, int32_t* __restrict__ idx,
                                                           double* __restrict__ mom, int64_t nblk) {
  __shared__ double sm[4 * MRI_MOM];
  if (icp_idle(status, max_iter)) return;
  const int64_t n = blockIdx.y;
  const int64_t lx = cloud_len(xl, n, P1), lt = cloud_len(yl, n, P2);
  const double m0 = xc[n * MRI_XC + 1], m1 = xc[n * MRI_XC + 2], m2 = xc[n * MRI_XC + 3];
  double a[MRI_MOM];
#pragma unroll
  for (int k = 0; k < MRI_MOM; ++k) a[k] = 0.0;
#pragma unroll
  for (int k = 0; k < MRR_PER; ++k) {
    const int64_t i = (int64_t)blockIdx.x * MRR_TILE + k * MRR_BLOCK + threadIdx.x;
    if (i >= P1) continue;
    int64_t j = -1;
    if (i < lx) {
      if (key) {
        const u64 kk = key[n * P1 + i];
        key[n * P1 + i] = ~0ull;
        j = (int64_t)key_index(kk);
      } else {
        j = i;
      }
      if (j >= lt) j = -1;  // no target (an empty target cloud leaves the key untouched)
    }
    if (idx) idx[n * P1 + i] = (int32_t)j;
    if (j < 0) continue;
    const double w = (double)point_weight(weights, n, P1, i, lx);
    const float* __restrict__ q = x + 3 * (n * P1 + i);
    const float* __restrict__ t = y + 3 * (n * P2 + j);
    const double y0 = (double)t[0], y1 = (double)t[1], y2 = (double)t[2];
    const double d0 = w * ((double)q[0] - m0), d1 = w * ((double)q[1] - m1), d2 = w * ((double)q[2] - m2);
    a[0] += w * y0;
    a[1] += w * y1;
    a[2] += w * y2;
    a[3] += d0 * y0;
    a[4] += d0 * y1;
    a[5] += d0 * y2;
    a[6] += d1 * y0;
    a[7] += d1 * y1;
    a[8] += d1 * y2;
    a[9] += d2 * y0;
    a[10] += d2 * y1;
    a[11] += d2 * y2;
  }
  block_sums<MRR_BLOCK / 64>(a, sm);
  if (threadIdx.x < MRI_MOM) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < MRI_MOM; ++k) v = threadIdx.x == k ? a[k] : v;
    mom[(n * nblk + blockIdx.x) * MRI_MOM + threadIdx.x] = v;
  }
}

__host__ __device__ __forceinline__ double det3(const double (&m)[3][3]) {
  return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
         m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

// The similarity transform of one cloud from its constants and its moment partials (summed in order), in float64:
// cov = sum w (x - mx)(y - my)^T / wc = U S V^T by a one-sided Jacobi (the columns of W = cov V are rotated until
// orthogonal: S = their norms, U = them normalised), R = U E V^T with E = diag(1, 1, det(U V^T)) unless
// reflections are allowed, s = tr(E S) / max(sum w |x - mx|^2 / wc, eps) or 1, T = my - s mx R. A cloud without
// weight gives the identity. (Also a host function, so that a CPU program can check the solve against LAPACK.)
__host__ __device__ void solve_cloud(const double* __restrict__ c, const double* __restrict__ mom, int64_t nblk, int flags,
                            double eps, float* out) {
  double m[MRI_MOM];
  for (int k = 0; k < MRI_MOM; ++k) m[k] = 0.0;
  for (int64_t b = 0; b < nblk; ++b)
    for (int k = 0; k < MRI_MOM; ++k) m[k] += mom[b * MRI_MOM + k];
  if (!(c[0] > 0.0)) {
    for (int k = 0; k < MRI_RTS; ++k) out[k] = (k == 0 || k == 4 || k == 8 || k == 12) ? 1.0f : 0.0f;
    return;
  }
  const double wc = c[0] > eps ? c[0] : eps;
  const double my[3] = {m[0] / wc, m[1] / wc, m[2] / wc};
  double W[3][3], V[3][3];
  double big = 0.0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      W[a][b] = (m[3 + 3 * a + b] - c[5 + a] * my[b]) / wc;
      V[a][b] = a == b ? 1.0 : 0.0;
      big = fabs(W[a][b]) > big ? fabs(W[a][b]) : big;
    }
  const double unit = (big > 0.0 && big < 1e300) ? big : 1.0;  // the rotations see entries of magnitude <= 1
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) W[a][b] /= unit;
  for (int sweep = 0; sweep < MRI_SWEEPS; ++sweep)
    for (int pr = 0; pr < 3; ++pr) {
      const int p = pr == 2 ? 1 : 0, q = pr == 0 ? 1 : 2;
      const double al = (W[0][p] * W[0][p] + W[1][p] * W[1][p]) + W[2][p] * W[2][p];
      const double be = (W[0][q] * W[0][q] + W[1][q] * W[1][q]) + W[2][q] * W[2][q];
      const double ga = (W[0][p] * W[0][q] + W[1][p] * W[1][q]) + W[2][p] * W[2][q];
      if (!(ga * ga > 1e-36 * (al * be))) continue;  // orthogonal already (or a zero column)
      const double ze = (be - al) / (2.0 * ga);
      const double tt = (ze >= 0.0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));
      const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
      for (int a = 0; a < 3; ++a) {
        const double wp = W[a][p], wq = W[a][q], vp = V[a][p], vq = V[a][q];
        W[a][p] = cs * wp - sn * wq;
        W[a][q] = sn * wp + cs * wq;
        V[a][p] = cs * vp - sn * vq;
        V[a][q] = sn * vp + cs * vq;
      }
    }
  double sg[3];
  for (int j = 0; j < 3; ++j) sg[j] = sqrt((W[0][j] * W[0][j] + W[1][j] * W[1][j]) + W[2][j] * W[2][j]);
  for (int pr = 0; pr < 3; ++pr) {  // descending singular values: (0,1), (1,2), (0,1)
    const int p = pr == 1 ? 1 : 0, q = p + 1;
    if (sg[p] < sg[q]) {
      const double ts = sg[p];
      sg[p] = sg[q];
      sg[q] = ts;
      for (int a = 0; a < 3; ++a) {
        const double tw = W[a][p], tv = V[a][p];
        W[a][p] = W[a][q];
        W[a][q] = tw;
        V[a][p] = V[a][q];
        V[a][q] = tv;
      }
    }
  }
  double U[3][3];
  const double tiny = 1e-13 * sg[0];
  if (sg[0] > 0.0) {
    for (int a = 0; a < 3; ++a) U[a][0] = W[a][0] / sg[0];
  } else {
    U[0][0] = 1.0;
    U[1][0] = U[2][0] = 0.0;
  }
  if (sg[1] > tiny) {
    for (int a = 0; a < 3; ++a) U[a][1] = W[a][1] / sg[1];
  } else {  // any unit vector orthogonal to the first: from the axis the first is least along
    int k = 0;
    if (fabs(U[1][0]) < fabs(U[k][0])) k = 1;
    if (fabs(U[2][0]) < fabs(U[k][0])) k = 2;
    double v[3], nn = 0.0;
    for (int a = 0; a < 3; ++a) {
      v[a] = (a == k ? 1.0 : 0.0) - U[k][0] * U[a][0];
      nn += v[a] * v[a];
    }
    nn = sqrt(nn);
    for (int a = 0; a < 3; ++a) U[a][1] = v[a] / nn;
  }
  if (sg[2] > tiny) {
    for (int a = 0; a < 3; ++a) U[a][2] = W[a][2] / sg[2];
  } else {
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  }
  const double e2 = (flags & MR_ICP_ALLOW_REFLECTION) ? 1.0 : (det3(U) * det3(V) < 0.0 ? -1.0 : 1.0);
  double R[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) R[a][b] = (U[a][0] * V[b][0] + U[a][1] * V[b][1]) + e2 * (U[a][2] * V[b][2]);
  double s = 1.0;
  if (flags & MR_ICP_ESTIMATE_SCALE) {
    const double xcov = c[4] / wc;
    s = (((sg[0] + sg[1]) + e2 * sg[2]) * unit) / (xcov > eps ? xcov : eps);
  }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) out[3 * a + b] = (float)R[a][b];
  for (int b = 0; b < 3; ++b) out[9 + b] = (float)(my[b] - s * ((c[1] * R[0][b] + c[2] * R[1][b]) + c[3] * R[2][b]));
  out[12] = (float)s;
}

// grid (nblk or 1, N). Thread 0 of every workgroup solves its cloud (the same inputs and code: the same bits in every
// workgroup of the cloud); workgroup 0 stores the transform in rts and, with hist, in slot status[1] of the history.
// res != NULL: the workgroup's tile of the residual sum w |s x R + T - y_nn|^2 with that transform.
__global__ void __launch_bounds__(MRR_BLOCK) k_icp_solve(const float* __restrict__ x, const float* __restrict__ y,
                                                         int64_t N, int64_t P1, int64_t P2,
                                                         const int64_t* __restrict__ xl,
                                                         const float* __restrict__ weights,
                                                         const double* __restrict__ xc, const double* __restrict__ mom,
                                                         int64_t nblk, const int32_t* __restrict__ idx, int flags,
                                                         double eps, const int32_t* __restrict__ status, int max_iter,
                                                         float* __restrict__ rts, float* __restrict__ hist,
                                                         double* __restrict__ res) {
  __shared__ double sm[4];
  __shared__ float tr[MRI_RTS];
  if (icp_idle(status, max_iter)) return;
  const int64_t n = blockIdx.y;
  if (threadIdx.x == 0) solve_cloud(xc + n * MRI_XC, mom + n * nblk * MRI_MOM, nblk, flags, eps, tr);
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x < MRI_RTS) {
    rts[n * MRI_RTS + threadIdx.x] = tr[threadIdx.x];
    if (hist) hist[((int64_t)status[1] * N + n) * MRI_RTS + threadIdx.x] = tr[threadIdx.x];
  }
  if (!res) return;
  const int64_t lx = cloud_len(xl, n, P1);
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < MRR_PER; ++k) {
    const int64_t i = (int64_t)blockIdx.x * MRR_TILE + k * MRR_BLOCK + threadIdx.x;
    if (i >= lx) continue;
    const int32_t j = idx[n * P1 + i];
    if (j < 0 || j >= P2) continue;
    const float* __restrict__ q = x + 3 * (n * P1 + i);
    const float* __restrict__ t = y + 3 * (n * P2 + j);
    float o0, o1, o2;
    sim_apply(tr, q[0], q[1], q[2], o0, o1, o2);
    const double d0 = (double)o0 - (double)t[0], d1 = (double)o1 - (double)t[1], d2 = (double)o2 - (double)t[2];
    acc += (double)point_weight(weights, n, P1, i, lx) * ((d0 * d0 + d1 * d1) + d2 * d2);
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) res[n * nblk + blockIdx.x] = acc;
}

// One workgroup: per cloud rmse = sqrt(residual / max(sum w, eps)) and its relative drop against the previous
// iteration's (float32; 1 on the first iteration, a NaN does not count as converged); then the status words.
// rmse holds the previous iteration's values on entry.
__global__ void __launch_bounds__(MRR_BLOCK) k_icp_status(const double* __restrict__ res, int64_t nblk, int64_t N,
                                                          const double* __restrict__ xc, double eps, float thr,
                                                          int max_iter, float* __restrict__ rmse,
                                                          int32_t* __restrict__ status) {
  __shared__ double sm[4];
  if (icp_idle(status, max_iter)) return;  // uniform
  const int it = status[1];
  double open = 0.0;
  for (int64_t n = threadIdx.x; n < N; n += MRR_BLOCK) {
    double s = 0.0;
    for (int64_t b = 0; b < nblk; ++b) s += res[n * nblk + b];
    const double wc = xc[n * MRI_XC] > eps ? xc[n * MRI_XC] : eps;
    const float r = (float)sqrt(s / wc);
    const float prev = rmse[n];
    const float rel = it == 0 ? 1.0f : (prev - r) / prev;
    if (!(rel <= thr)) open += 1.0;
    rmse[n] = r;
  }
  open = block_sum(open, sm);  // also orders every thread's read of status[1] before its update
  if (threadIdx.x == 0) {
    status[1] = it + 1;
    if (open == 0.0) status[0] = 1;
  }
}

// out[n, i] = s (x[n, i] R) + T for every entry of the padded tensor.
__global__ void __launch_bounds__(MRR_BLOCK) k_icp_apply(const float* __restrict__ x, int64_t P,
                                                         const float* __restrict__ rts, float* __restrict__ out) {
  const int64_t n = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * MRR_BLOCK + threadIdx.x;
  if (i >= P) return;
  const float* __restrict__ q = x + 3 * (n * P + i);
  float o0, o1, o2;
  sim_apply(rts + n * MRI_RTS, q[0], q[1], q[2], o0, o1, o2);
  float* __restrict__ o = out + 3 * (n * P + i);
  o[0] = o0;
  o[1] = o1;
  o[2] = o2;
}

// ---------------------------------------------------------------------------
// Point-to-plane ICP (mr_icp_plane_iterate): a second estimator on the loop above. k_icp_nn is launched as it is;
// k_icp_plane_moments sums the Gauss-Newton normal equations of the valid pairs, k_icp_plane_solve takes one damped
// step about the transformed source mean and sums the new residual, k_icp_plane_status divides by the pair count.
// The rule is stated in include/mi355r.h; everything but the moments kernel is in mr_icp.h.
// ---------------------------------------------------------------------------
// grid (nblk, N), k_icp_moments' layout: a tile of source points. Decodes key -> (distance, index) and sets the key
// back to all-ones; a pair is valid when the index is inside the target and the distance is <= max_dist2 (+inf: every
// pair); idx gets the index, -1 for no valid pair. Per valid pair, p = sim_apply(x_i), q = y_j, n = yn_j:
// r = (p - q).n, J = [(p - c) x n, n], and the workgroup's sums of J J^T (upper triangle), J r and 1 go to pmom.
// Workgroup 0 of a cloud also copies the transform to prev for k_icp_plane_solve.
__global__ void __launch_bounds__(MRR_BLOCK) k_icp_plane_moments(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ yn, int64_t P1, int64_t P2,
    const int64_t* __restrict__ xl, const int64_t* __restrict__ yl, const double* __restrict__ xc,
    const float* __restrict__ rts, float max_dist2, const int32_t* __restrict__ status, int max_iter,
    u64* __restrict__ key, int32_t* __restrict__ idx, float* __restrict__ prev, double* __restrict__ pmom,
    int64_t nblk) {
  __shared__ double sm[4 * MRI_PMOM];
  if (icp_idle(status, max_iter)) return;
  const int64_t n = blockIdx.y;
  const int64_t lx = cloud_len(xl, n, P1), lt = cloud_len(yl, n, P2);
  const float* __restrict__ tr = rts + n * MRI_RTS;
  if (blockIdx.x == 0 && threadIdx.x < MRI_RTS) prev[n * MRI_RTS + threadIdx.x] = tr[threadIdx.x];
  double c[3];
  plane_centre(xc + n * MRI_XC, tr, c);
  const bool every = max_dist2 == __builtin_inff();
  double a[MRI_PMOM];
#pragma unroll
  for (int k = 0; k < MRI_PMOM; ++k) a[k] = 0.0;
#pragma unroll
  for (int k = 0; k < MRR_PER; ++k) {
    const int64_t i = (int64_t)blockIdx.x * MRR_TILE + k * MRR_BLOCK + threadIdx.x;
    if (i >= P1) continue;
    int64_t j = -1;
    if (i < lx) {
      const u64 kk = key[n * P1 + i];
      key[n * P1 + i] = ~0ull;
      j = (int64_t)key_index(kk);
      if (j >= lt || !(every || key_dist(kk) <= max_dist2)) j = -1;  // an empty target leaves the key untouched
    }
    idx[n * P1 + i] = (int32_t)j;
    if (j < 0) continue;
    const float* __restrict__ q = x + 3 * (n * P1 + i);
    const float* __restrict__ t = y + 3 * (n * P2 + j);
    const float* __restrict__ nn = yn + 3 * (n * P2 + j);
    float p0, p1, p2;
    sim_apply(tr, q[0], q[1], q[2], p0, p1, p2);
    plane_accum(p0, p1, p2, t, nn, c, a);
  }
  plane_store(a, sm, pmom, n, nblk);
}

// ---------------------------------------------------------------------------
// Chamfer distance of ONE cloud pair under S rigid / similarity poses (mr_posed_chamfer): x' = s (x R) + T per pose.
// ---------------------------------------------------------------------------
#define MRP_MOM 13     // per-workgroup pose moments (double): sum g (3), sum x^T g (9, row = x component), sum (x R).g

struct PosedWS {
  double* part;   // (2, S, ntile) distance sums of a workgroup's queries
  double* mom;    // (2, S, ntile, MRP_MOM)
  int64_t ntile;  // query tiles of the larger cloud
  size_t bytes;
};
PosedWS carve_posed(void* base, int64_t S, int64_t P1, int64_t P2) {
  PosedWS w;
  Carver c(base);
  w.ntile = ceil_div(P1 > P2 ? P1 : P2, MRN_QT);
  w.part = c.take<double>(2 * (size_t)(S * w.ntile));
  w.mom = c.take<double>(2 * (size_t)(S * w.ntile) * MRP_MOM);
  w.bytes = c.off;
  return w;
}

// grid (query tiles of the larger cloud, S, directions). A workgroup owns one pose, one direction and one tile of
// 512 queries and scans ALL targets itself, in ascending LDS chunks: with the strict < its minimum is final and
// ties go to the lowest index, so there is no key buffer, memset, atomic or decode pass. Direction 0: queries x'
// (x transformed in registers, as k_icp_nn), targets y. Direction 1: queries y, targets x' transformed while they
// are staged: the same sim_apply, so both directions see the bits a materialised cloud would hold. Outputs per
// workgroup: idx (optional), the float64 sum of its queries' distances, and (mom != NULL) the pose moments with
// g = x' - y of every pair (sign(.) for norm 1) and x the pair's untransformed source point.
// Norm 2 is held at the 4 waves per SIMD it has always run at (97-128 VGPRs; 8 workgroups = 16 waves per CU, 4 on
// every SIMD). At <= 96 VGPRs the LDS admits a ninth workgroup, whose 2 waves load the four SIMDs 5, 5, 4, 4, and
// the VALU-bound scan ran 11 % slower at S = 1000, P = 1000 / 495 (profiles/nn_scan_ab.json). Norm 1 is as it was.
template <int NORM>
__global__ void __launch_bounds__(MRN_BLOCK) __attribute__((amdgpu_waves_per_eu(4, NORM == 2 ? 4 : 8))) k_posed_nn(
    const float* __restrict__ x, const float* __restrict__ y, int64_t P1, int64_t P2, const float* __restrict__ rts,
    int64_t S, int64_t ntile, int32_t* __restrict__ idx_x, int32_t* __restrict__ idx_y, double* __restrict__ part,
    double* __restrict__ mom) {
  __shared__ float4 sm[MRN_MAXCHUNK];
  __shared__ double red[2 * MRP_MOM];
  const int d = blockIdx.z;
  const int64_t n = blockIdx.y;
  const int64_t Pq = d ? P2 : P1, Pt = d ? P1 : P2;
  const int64_t q0 = (int64_t)blockIdx.x * MRN_QT;
  if (q0 >= Pq) return;  // uniform over the workgroup
  const float* __restrict__ q = d ? y : x;
  const float* __restrict__ t = d ? x : y;
  const float* __restrict__ tr = rts + n * MRI_RTS;

  float qx[MRN_Q], qy[MRN_Q], qz[MRN_Q], best[MRN_Q];
  int bi[MRN_Q];
  scan_load_queries(q, q0, Pq, tr, d == 0, qx, qy, qz);
#pragma unroll
  for (int k = 0; k < MRN_Q; ++k) {
    best[k] = __builtin_inff();
    bi[k] = 0;
  }
  for (int64_t t0 = 0; t0 < Pt; t0 += MRN_MAXCHUNK) {
    const int cnt = (int)((Pt - t0 < MRN_MAXCHUNK) ? Pt - t0 : MRN_MAXCHUNK);
    if (t0) __syncthreads();  // the previous chunk has been read
    scan_stage(sm, t, t0, cnt, tr, d != 0);
    __syncthreads();
    scan_nearest<NORM>(sm, cnt, (int)t0, qx, qy, qz, best, bi);
  }

  int32_t* __restrict__ idx = d ? idx_y : idx_x;
  double a[MRP_MOM];
#pragma unroll
  for (int k = 0; k < MRP_MOM; ++k) a[k] = 0.0;
  double dsum = 0.0;
#pragma unroll
  for (int k = 0; k < MRN_Q; ++k) {
    const int64_t i = q0 + k * MRN_BLOCK + threadIdx.x;
    if (i >= Pq) continue;
    if (idx) idx[n * Pq + i] = bi[k];
    dsum += (double)best[k];
    if (!mom) continue;
    // the pair's source point (untransformed), its image x' and the point of y
    const float* __restrict__ sp = x + 3 * (d ? (int64_t)bi[k] : i);
    const float s0 = sp[0], s1 = sp[1], s2 = sp[2];
    float g0, g1, g2;
    if (d == 0) {
      const float* __restrict__ tp = y + 3 * (int64_t)bi[k];
      g0 = qx[k] - tp[0];
      g1 = qy[k] - tp[1];
      g2 = qz[k] - tp[2];
    } else {
      float o0, o1, o2;
      sim_apply(tr, s0, s1, s2, o0, o1, o2);
      g0 = o0 - qx[k];
      g1 = o1 - qy[k];
      g2 = o2 - qz[k];
    }
    if (NORM == 1) {
      g0 = sgn(g0);
      g1 = sgn(g1);
      g2 = sgn(g2);
    }
    const double e0 = (double)g0, e1 = (double)g1, e2 = (double)g2;
    const double x0 = (double)s0, x1 = (double)s1, x2 = (double)s2;
    a[0] += e0;
    a[1] += e1;
    a[2] += e2;
    a[3] += x0 * e0;
    a[4] += x0 * e1;
    a[5] += x0 * e2;
    a[6] += x1 * e0;
    a[7] += x1 * e1;
    a[8] += x1 * e2;
    a[9] += x2 * e0;
    a[10] += x2 * e1;
    a[11] += x2 * e2;
    const double r0 = (x0 * (double)tr[0] + x1 * (double)tr[3]) + x2 * (double)tr[6];
    const double r1 = (x0 * (double)tr[1] + x1 * (double)tr[4]) + x2 * (double)tr[7];
    const double r2 = (x0 * (double)tr[2] + x1 * (double)tr[5]) + x2 * (double)tr[8];
    a[12] += (r0 * e0 + r1 * e1) + r2 * e2;
  }
  const int64_t slot = ((int64_t)d * S + n) * ntile + blockIdx.x;
  {
    double one[1] = {dsum};
    block_sums<MRN_BLOCK / 64>(one, red);
    if (threadIdx.x == 0) part[slot] = one[0];
  }
  if (!mom) return;  // uniform
  block_sums<MRN_BLOCK / 64>(a, red);
  if (threadIdx.x < MRP_MOM) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < MRP_MOM; ++k) v = threadIdx.x == k ? a[k] : v;
    mom[slot * MRP_MOM + threadIdx.x] = v;
  }
}

// Thread n finishes pose n: its tiles' partials in order, the point reduction, x -> y plus y -> x (x -> y alone with
// MR_CHAMFER_SINGLE) as k_cham_final does; pose_grad (S, 13; may be NULL) = d out[n] / d (R, T, s) in rts' layout
// from the moments: dT = k sum_d c_d sum g, dR = k s sum_d c_d sum x^T g, ds = k sum_d c_d sum (x R).g, k = 2 or 1.
__global__ void __launch_bounds__(MRR_BLOCK) k_posed_final(const double* __restrict__ part,
                                                           const double* __restrict__ mom, int64_t ntile, int64_t S,
                                                           int64_t P1, int64_t P2, const float* __restrict__ rts,
                                                           int norm, int flags, float* __restrict__ out,
                                                           float* __restrict__ pose_grad) {
  const int64_t n = (int64_t)blockIdx.x * MRR_BLOCK + threadIdx.x;
  if (n >= S) return;
  const bool single = flags & MR_CHAMFER_SINGLE, pmean = flags & MR_CHAMFER_POINT_MEAN;
  double v = 0.0;
  double m[MRP_MOM];
#pragma unroll
  for (int k = 0; k < MRP_MOM; ++k) m[k] = 0.0;
  for (int d = 0; d < (single ? 1 : 2); ++d) {
    const int64_t Pq = d ? P2 : P1;
    const int64_t tiles = (Pq + MRN_QT - 1) / MRN_QT;
    const double c = pmean ? 1.0 / (double)(Pq > 1 ? Pq : 1) : 1.0;
    const int64_t slot = ((int64_t)d * S + n) * ntile;
    double s = 0.0;
    for (int64_t b = 0; b < tiles; ++b) s += part[slot + b];
    v += c * s;
    if (pose_grad) {
      double md[MRP_MOM];
#pragma unroll
      for (int k = 0; k < MRP_MOM; ++k) md[k] = 0.0;
      for (int64_t b = 0; b < tiles; ++b)
#pragma unroll
        for (int k = 0; k < MRP_MOM; ++k) md[k] += mom[(slot + b) * MRP_MOM + k];
#pragma unroll
      for (int k = 0; k < MRP_MOM; ++k) m[k] += c * md[k];
    }
  }
  out[n] = (float)v;
  if (!pose_grad) return;
  const double kf = norm == 2 ? 2.0 : 1.0;
  const double ks = kf * (double)rts[n * MRI_RTS + 12];
  float* __restrict__ o = pose_grad + n * MRI_RTS;
#pragma unroll
  for (int k = 0; k < 9; ++k) o[k] = (float)(ks * m[3 + k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) o[9 + k] = (float)(kf * m[k]);
  o[12] = (float)(kf * m[12]);
}

// ---------------------------------------------------------------------------
// Host side of the ICP loops: the argument checks and the iterations, which take their search as a launch.
// ---------------------------------------------------------------------------
int check_icp(const char* who, const float* x, int64_t N, int64_t P1, int64_t P2) {
  if (int rc = check_sizes(who, N, P1, P2)) return rc;
  if (!x) return set_err(MR_EINVAL, "%s: x is NULL", who);
  return MR_OK;
}

// What mr_icp_iterate and mr_icp_iterate_grid check first.
int check_icp_iterate(const char* who, const float* x, const float* y, int64_t N, int64_t P1, int64_t P2,
                      int32_t flags, int32_t max_iterations, int32_t iterations, const float* rts,
                      const float* history, const float* rmse, const int32_t* status, const void* ws) {
  if (int rc = check_icp(who, x, N, P1, P2)) return rc;
  if (flags & ~MR_ICP_ALL) return set_err(MR_EINVAL, "%s: unknown bits in flags", who);
  if (max_iterations < 1 || iterations < 0 || (int64_t)max_iterations * N > (1ll << 40) / MRI_RTS)
    return set_err(MR_EINVAL, "%s: max_iterations must be >= 1 (and the history addressable), iterations >= 0", who);
  if (!y || !rts || !history || !rmse || !status || !ws) return set_err(MR_EINVAL, "%s: NULL pointer", who);
  return MR_OK;
}

// The grid argument of the *_iterate_grid entry points, mr_knn_points_grid's contract: after the sizes are known good.
int check_icp_grid(const char* who, const void* grid, size_t grid_bytes, int64_t N, int64_t P2, GridBuf& b) {
  if (!grid) return set_err(MR_EINVAL, "%s: grid is NULL", who);
  b = carve_grid(grid, N, P2);
  if (grid_bytes < b.bytes) return set_err(MR_EWORKSPACE, "%s: grid buffer too small", who);
  return MR_OK;
}

// The launch of k_icp_nn_grid for a batch, as the search of an iteration.
struct GridSearch {
  const float* x;
  int64_t N, P1, P2;
  const int64_t *xl, *yl;
  GridBuf b;
  const float* rts;
  float max_dist2;  // +inf: no cap
  const int32_t* status;
  int max_iter;
  u64 *key, *visited;
  hipStream_t st;
  int operator()() const {
    const dim3 g((unsigned)ceil_div(P1, MRG_QBLOCK), (unsigned)N);
    return launch(KID_NONE, "k_icp_nn_grid", max_dist2 < __builtin_inff() ? k_icp_nn_grid<true> : k_icp_nn_grid<false>, g,
                  MRG_QBLOCK, 0, st, x, P1, P2, xl, yl, grid_budget(P2), (const GridHead*)b.head,
                  (const uint32_t*)b.cell_start, (const float4*)b.pts, rts, max_dist2, status, max_iter, key, visited);
  }
};

// The launch of k_icp_nn for a batch, as the search of an iteration.
struct ScanSearch {
  const float *x, *y;
  NNGeom g;
  const int64_t *xl, *yl;
  const float* rts;
  const int32_t* status;
  int max_iter;
  u64* key;
  hipStream_t st;
  int operator()() const {
    return launch(KID_NONE, "k_icp_nn", k_icp_nn, dim3((unsigned)g.groups[0], (unsigned)g.N), MRN_BLOCK, 0, st, x, y, g,
                  xl, yl, rts, status, max_iter, key);
  }
};

// `iterations` iterations of the point-to-point loop: `search` leaves every source point's key in w.key, the moments,
// solve and status launches follow.
template <class Search>
int icp_iterations(const Search& search, const float* x, const float* y, int64_t N, int64_t P1, int64_t P2,
                   const int64_t* x_lengths, const int64_t* y_lengths, int32_t flags, float relative_rmse_thr,
                   int32_t max_iterations, int32_t iterations, float* rts, float* history, float* rmse,
                   int32_t* status, const IcpWS& w, hipStream_t st) {
  const dim3 gt((unsigned)w.nblk, (unsigned)N);
  for (int it = 0; it < iterations; ++it) {
    if (int rc = search()) return rc;
    if (int rc = launch(KID_NONE, "k_icp_moments", k_icp_moments, gt, MRR_BLOCK, 0, st, x, y, P1, P2, x_lengths, y_lengths,
                        (const float*)nullptr, (const double*)w.xc, (const int32_t*)status, max_iterations, w.key, w.idx,
                        w.mom, w.nblk))
      return rc;
    if (int rc = launch(KID_NONE, "k_icp_solve", k_icp_solve, gt, MRR_BLOCK, 0, st, x, y, N, P1, P2, x_lengths,
                        (const float*)nullptr, (const double*)w.xc, (const double*)w.mom, w.nblk, (const int32_t*)w.idx,
                        flags, 1e-9, (const int32_t*)status, max_iterations, rts, history, w.res))
      return rc;
    if (int rc = launch(KID_NONE, "k_icp_status", k_icp_status, 1, MRR_BLOCK, 0, st, (const double*)w.res, w.nblk, N,
                        (const double*)w.xc, 1e-9, relative_rmse_thr, max_iterations, rmse, status))
      return rc;
  }
  return MR_OK;
}

// What mr_icp_plane_iterate and mr_icp_plane_iterate_grid check first.
int check_icp_plane_iterate(const char* who, const float* x, const float* y, const float* y_normals, int64_t N,
                            int64_t P1, int64_t P2, float max_dist2, int32_t max_iterations, int32_t iterations,
                            const float* rts, const float* history, const float* rmse, const int32_t* status,
                            const void* ws) {
  if (int rc = check_icp(who, x, N, P1, P2)) return rc;
  if (!(max_dist2 > 0.0f)) return set_err(MR_EINVAL, "%s: max_dist2 must be > 0 (+inf: no limit)", who);
  if (max_iterations < 1 || iterations < 0 || (int64_t)max_iterations * N > (1ll << 40) / MRI_RTS)
    return set_err(MR_EINVAL, "%s: max_iterations must be >= 1 (and the history addressable), iterations >= 0", who);
  if (!y || !y_normals || !rts || !history || !rmse || !status || !ws) return set_err(MR_EINVAL, "%s: NULL pointer", who);
  return MR_OK;
}

// `iterations` iterations of the point-to-plane loop: `search` leaves every source point's key in w.icp.key, the
// moments, solve and status launches follow.
template <class Search>
int icp_plane_iterations(const Search& search, const float* x, const float* y, const float* y_normals, int64_t N,
                         int64_t P1, int64_t P2, const int64_t* x_lengths, const int64_t* y_lengths,
                         float max_dist2, float relative_rmse_thr, int32_t max_iterations, int32_t iterations,
                         float* rts, float* history, float* rmse, int32_t* status, const IcpPlaneWS& w,
                         hipStream_t st) {
  const dim3 gt((unsigned)w.icp.nblk, (unsigned)N);
  for (int it = 0; it < iterations; ++it) {
    if (int rc = search()) return rc;
    if (int rc = launch(KID_NONE, "k_icp_plane_moments", k_icp_plane_moments, gt, MRR_BLOCK, 0, st, x, y, y_normals, P1, P2,
                        x_lengths, y_lengths, (const double*)w.icp.xc, (const float*)rts, max_dist2,
                        (const int32_t*)status, max_iterations, w.icp.key, w.icp.idx, w.prev, w.pmom, w.icp.nblk))
      return rc;
    if (int rc = launch(KID_NONE, "k_icp_plane_solve", k_icp_plane_solve, gt, MRR_BLOCK, 0, st, x, y, y_normals, N, P1, P2,
                        x_lengths, (const double*)w.icp.xc, (const double*)w.pmom, w.icp.nblk,
                        (const int32_t*)w.icp.idx, (const float*)w.prev, (const int32_t*)status, max_iterations, rts,
                        history, w.cnt, w.icp.res))
      return rc;
    if (int rc = launch(KID_NONE, "k_icp_plane_status", k_icp_plane_status, 1, MRR_BLOCK, 0, st, (const double*)w.icp.res,
                        w.icp.nblk, N, (const double*)w.cnt, relative_rmse_thr, max_iterations, rmse, status))
      return rc;
  }
  return MR_OK;
}

}  // namespace

extern "C" {

size_t mr_posed_chamfer_workspace(int64_t S, int64_t P1, int64_t P2) {
  if (!sizes_ok(S, P1, P2)) return 0;
  return carve_posed(nullptr, S, P1, P2).bytes;
}

int32_t mr_posed_chamfer(const float* x, const float* y, int64_t P1, int64_t P2, const float* rts, int64_t S,
                         int32_t norm, int32_t flags, float* out, int32_t* idx_x, int32_t* idx_y, float* pose_grad,
                         void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_clouds("posed chamfer", x, y, S, P1, P2, norm)) return rc;
  if (flags & ~(MR_CHAMFER_POINT_MEAN | MR_CHAMFER_SINGLE))
    return set_err(MR_EINVAL, "posed chamfer: flags takes MR_CHAMFER_POINT_MEAN and MR_CHAMFER_SINGLE only");
  if (!rts || !out || !ws) return set_err(MR_EINVAL, "posed chamfer: rts / out / workspace is NULL");
  const PosedWS w = carve_posed(ws, S, P1, P2);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "posed chamfer workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  const bool single = flags & MR_CHAMFER_SINGLE;
  // a single-directional call scans (and writes idx for) x -> y alone: its grid covers the tiles of x
  const int64_t gx = single ? (int64_t)ceil_div(P1, MRN_QT) : w.ntile;
  const dim3 grid((unsigned)gx, (unsigned)S, single ? 1u : 2u);
  double* mom = pose_grad ? w.mom : nullptr;
  if (int rc = launch(KID_NONE, "k_posed_nn", norm == 2 ? k_posed_nn<2> : k_posed_nn<1>, grid, MRN_BLOCK, 0, st, x, y, P1, P2,
                      rts, S, w.ntile, idx_x, idx_y, w.part, mom))
    return rc;
  return launch(KID_NONE, "k_posed_final", k_posed_final, (unsigned)ceil_div(S, MRR_BLOCK), MRR_BLOCK, 0, st,
                (const double*)w.part, (const double*)mom, w.ntile, S, P1, P2, rts, (int)norm, (int)flags, out, pose_grad);
}

size_t mr_nearest_points_workspace(int64_t N, int64_t P1, int64_t P2) {
  if (!sizes_ok(N, P1, P2)) return 0;
  return carve_points(nullptr, N, P1, P2).bytes;
}

int32_t mr_nearest_points(const float* x, const float* y, int64_t N, int64_t P1, int64_t P2, const int64_t* x_lengths,
                          const int64_t* y_lengths, int32_t norm, float* dist_x, int32_t* idx_x, float* dist_y,
                          int32_t* idx_y, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_clouds("nearest points", x, y, N, P1, P2, norm)) return rc;
  if (!dist_x || !idx_x || !dist_y || !idx_y || !ws)
    return set_err(MR_EINVAL, "nearest points: an output or the workspace is NULL");
  const PointsWS w = carve_points(ws, N, P1, P2);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "nearest points workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  const NNGeom g = nn_geom(N, P1, P2);
  if (int rc = run_nn(x, y, g, x_lengths, y_lengths, norm, 2, w, st)) return rc;
  return launch(KID_NONE, "k_nn_reduce", k_nn_reduce, dim3((unsigned)w.nblk, (unsigned)N, 2), MRR_BLOCK, 0, st, g, x_lengths,
                y_lengths, w.key[0], w.key[1], dist_x, idx_x, dist_y, idx_y, nullptr, w.nblk);
}

size_t mr_chamfer_workspace(int64_t N, int64_t P1, int64_t P2) { return mr_nearest_points_workspace(N, P1, P2); }

int32_t mr_chamfer_forward(const float* x, const float* y, int64_t N, int64_t P1, int64_t P2, const int64_t* x_lengths,
                           const int64_t* y_lengths, const float* weights, int32_t norm, int32_t flags, int32_t* idx_x,
                           int32_t* idx_y, float* coef, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_clouds("chamfer", x, y, N, P1, P2, norm)) return rc;
  if ((flags & ~MR_CHAMFER_ALL) || ((flags & MR_CHAMFER_BATCH_MEAN) && (flags & MR_CHAMFER_BATCH_SUM)))
    return set_err(MR_EINVAL, "chamfer: unknown or contradictory bits in flags");
  if (!out || !ws) return set_err(MR_EINVAL, "chamfer: out / workspace is NULL");
  const PointsWS w = carve_points(ws, N, P1, P2);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "chamfer workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  const int dirs = (flags & MR_CHAMFER_SINGLE) ? 1 : 2;
  const NNGeom g = nn_geom(N, P1, P2);
  if (int rc = run_nn(x, y, g, x_lengths, y_lengths, norm, dirs, w, st)) return rc;
  if (int rc = launch(KID_NONE, "k_nn_reduce", k_nn_reduce, dim3((unsigned)w.nblk, (unsigned)N, (unsigned)dirs), MRR_BLOCK, 0,
                      st, g, x_lengths, y_lengths, w.key[0], w.key[1], nullptr, idx_x, nullptr, idx_y, w.part, w.nblk))
    return rc;
  return launch(KID_NONE, "k_cham_final", k_cham_final, 1, MRR_BLOCK, 0, st, w.part, w.nblk, N, P1, P2, x_lengths, y_lengths,
                weights, flags, out, coef);
}

size_t mr_chamfer_backward_workspace(int64_t N, int64_t P1, int64_t P2) {
  if (!sizes_ok(N, P1, P2)) return 0;
  return carve_fix(nullptr, 3 * N * (P1 + P2)).bytes;
}

int32_t mr_chamfer_backward(const float* x, const float* y, int64_t N, int64_t P1, int64_t P2, int32_t norm,
                            int32_t flags, const int32_t* idx_x, const int32_t* idx_y, const float* coef,
                            const float* grad_out, float* grad_x, float* grad_y, void* ws, size_t ws_bytes,
                            void* stream) {
  if (int rc = check_clouds("chamfer backward", x, y, N, P1, P2, norm)) return rc;
  if (flags & ~MR_CHAMFER_ALL) return set_err(MR_EINVAL, "chamfer backward: unknown bits in flags");
  const bool single = flags & MR_CHAMFER_SINGLE;
  if (!idx_x || (!single && !idx_y) || !coef || !grad_out || !grad_x || !grad_y || !ws)
    return set_err(MR_EINVAL, "chamfer backward: NULL pointer");
  const FixWS w = carve_fix(ws, 3 * N * (P1 + P2));
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "chamfer backward workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  if (single) idx_y = nullptr;
  if (int rc = memset_async(ws, 0, w.bytes, st)) return rc;
  const int per_cloud = !(flags & (MR_CHAMFER_BATCH_MEAN | MR_CHAMFER_BATCH_SUM));
  const unsigned nb = ceil_div(P1 > P2 ? P1 : P2, MRR_BLOCK);
  const dim3 gs(nb, (unsigned)N, single ? 1u : 2u), gg(nb, (unsigned)N, 2u);
  if (int rc = launch(KID_NONE, "k_cham_scatter", norm == 2 ? k_cham_scatter<2> : k_cham_scatter<1>, gs, MRR_BLOCK, 0, st, x, y,
                      N, P1, P2, idx_x, idx_y, w.fix, w.rem))
    return rc;
  return launch(KID_NONE, "k_cham_grad", norm == 2 ? k_cham_grad<2> : k_cham_grad<1>, gg, MRR_BLOCK, 0, st, x, y, N, P1, P2,
                idx_x, idx_y, coef, grad_out, per_cloud, w.fix, w.rem, grad_x, grad_y);
}

int32_t mr_sample_points_forward(const float* verts, int64_t V, const int32_t* faces, int64_t F,
                                 const int32_t* face_idx, const float* uv, int64_t M, float* points, void* stream) {
  if (!mesh_sizes_ok(V, F, M)) return set_err(MR_EINVAL, "sample points: V, F or the sample count out of range");
  if (M == 0) return MR_OK;
  if (!face_idx || !uv || !points || (F > 0 && (!faces || !verts)))
    return set_err(MR_EINVAL, "sample points: NULL pointer");
  return launch(KID_NONE, "k_sample_fwd", k_sample_fwd, ceil_div(M, MRR_BLOCK), MRR_BLOCK, 0, (hipStream_t)stream, verts, V,
                faces, F, face_idx, uv, M, points);
}

size_t mr_sample_points_backward_workspace(int64_t V) {
  if (!mesh_sizes_ok(V, 0, 0)) return 0;
  return carve_fix(nullptr, 3 * V).bytes;
}

int32_t mr_sample_points_backward(int64_t V, const int32_t* faces, int64_t F, const int32_t* face_idx, const float* uv,
                                  int64_t M, const float* grad_points, float* grad_verts, void* ws, size_t ws_bytes,
                                  void* stream) {
  if (!mesh_sizes_ok(V, F, M)) return set_err(MR_EINVAL, "sample points: V, F or the sample count out of range");
  if (V == 0) return MR_OK;
  if (!grad_verts || !ws || (M > 0 && (!face_idx || !uv || !grad_points)) || (F > 0 && !faces))
    return set_err(MR_EINVAL, "sample points backward: NULL pointer");
  const FixWS w = carve_fix(ws, 3 * V);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "sample points backward workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  if (int rc = memset_async(ws, 0, w.bytes, st)) return rc;
  if (M > 0 && F > 0)
    if (int rc = launch(KID_NONE, "k_sample_scatter", k_sample_scatter, ceil_div(M, MRR_BLOCK), MRR_BLOCK, 0, st, V, faces, F,
                        face_idx, uv, M, grad_points, w.fix, w.rem))
      return rc;
  return launch(KID_NONE, "k_fix_to_float", k_fix_to_float, ceil_div(3 * V, MRR_BLOCK), MRR_BLOCK, 0, st, w.fix, w.rem, 3 * V,
                grad_verts);
}

int32_t mr_face_areas(const float* verts, int64_t V, const int32_t* faces, int64_t F, float* areas, void* stream) {
  if (!mesh_sizes_ok(V, F, 0)) return set_err(MR_EINVAL, "face areas: V or F out of range");
  if (F == 0) return MR_OK;
  if (!verts || !faces || !areas) return set_err(MR_EINVAL, "face areas: NULL pointer");
  return launch(KID_NONE, "k_face_areas", k_face_areas, ceil_div(F, MRR_BLOCK), MRR_BLOCK, 0, (hipStream_t)stream, verts, V,
                faces, F, areas);
}

size_t mr_icp_workspace(int64_t N, int64_t P1, int64_t P2) {
  if (!sizes_ok(N, P1, P2)) return 0;
  return carve_icp(nullptr, N, P1).bytes;
}

int32_t mr_icp_init(const float* x, int64_t N, int64_t P1, int64_t P2, const int64_t* x_lengths, const float* R0,
                    const float* T0, const float* s0, float* rts, int32_t* status, void* ws, size_t ws_bytes,
                    void* stream) {
  if (int rc = check_icp("icp init", x, N, P1, P2)) return rc;
  if (!rts || !status || !ws) return set_err(MR_EINVAL, "icp init: rts / status / workspace is NULL");
  if ((R0 || T0 || s0) && !(R0 && T0 && s0)) return set_err(MR_EINVAL, "icp init: R0, T0 and s0 go together");
  const IcpWS w = carve_icp(ws, N, P1);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "icp workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  if (int rc = memset_async(w.key, 0xff, w.key_bytes, st)) return rc;
  if (int rc = memset_async(status, 0, 2 * sizeof(int32_t), st)) return rc;
  return launch(KID_NONE, "k_icp_xstats", k_icp_xstats, (unsigned)N, MRR_BLOCK, 0, st, x, P1, x_lengths, (const float*)nullptr,
                1e-9, w.xc, R0, T0, s0, rts);
}

int32_t mr_icp_iterate(const float* x, const float* y, int64_t N, int64_t P1, int64_t P2, const int64_t* x_lengths,
                       const int64_t* y_lengths, int32_t flags, float relative_rmse_thr, int32_t max_iterations,
                       int32_t iterations, float* rts, float* history, float* rmse, int32_t* status, void* ws,
                       size_t ws_bytes, void* stream) {
  if (int rc = check_icp_iterate("icp", x, y, N, P1, P2, flags, max_iterations, iterations, rts, history, rmse, status, ws))
    return rc;
  const IcpWS w = carve_icp(ws, N, P1);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "icp workspace too small");
  const NNGeom g = nn_geom(N, P1, P2, MRI_WANT_GROUPS);
  if (g.groups[0] > 0x7fffffffll) return set_err(MR_EUNSUPPORTED, "icp: P1 * P2 is too large for one launch");
  const hipStream_t st = (hipStream_t)stream;
  const ScanSearch search{x, y, g, x_lengths, y_lengths, rts, status, max_iterations, w.key, st};
  return icp_iterations(search, x, y, N, P1, P2, x_lengths, y_lengths, flags, relative_rmse_thr, max_iterations,
                        iterations, rts, history, rmse, status, w, st);
}

int32_t mr_icp_iterate_grid(const float* x, const float* y, int64_t N, int64_t P1, int64_t P2, const int64_t* x_lengths,
                            const int64_t* y_lengths, const void* grid, size_t grid_bytes, int32_t flags,
                            float relative_rmse_thr, int32_t max_iterations, int32_t iterations, float* rts,
                            float* history, float* rmse, int32_t* status, uint64_t* visited, void* ws, size_t ws_bytes,
                            void* stream) {
  if (int rc = check_icp_iterate("icp grid", x, y, N, P1, P2, flags, max_iterations, iterations, rts, history, rmse, status,
                                 ws))
    return rc;
  GridBuf b;
  if (int rc = check_icp_grid("icp grid", grid, grid_bytes, N, P2, b)) return rc;
  const IcpWS w = carve_icp(ws, N, P1);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "icp grid: icp workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  const GridSearch search{x, N, P1, P2, x_lengths, y_lengths, b, rts, __builtin_inff(), status, max_iterations, w.key,
                          (u64*)visited, st};
  return icp_iterations(search, x, y, N, P1, P2, x_lengths, y_lengths, flags, relative_rmse_thr, max_iterations,
                        iterations, rts, history, rmse, status, w, st);
}

int32_t mr_icp_transform(const float* x, int64_t N, int64_t P, const float* rts, float* out, void* stream) {
  if (int rc = check_icp("icp transform", x, N, P, 1)) return rc;
  if (!rts || !out) return set_err(MR_EINVAL, "icp transform: rts / out is NULL");
  return launch(KID_NONE, "k_icp_apply", k_icp_apply, dim3((unsigned)ceil_div(P, MRR_BLOCK), (unsigned)N), MRR_BLOCK, 0,
                (hipStream_t)stream, x, P, rts, out);
}

size_t mr_icp_plane_workspace(int64_t N, int64_t P1, int64_t P2) {
  if (!sizes_ok(N, P1, P2)) return 0;
  return carve_icp_plane(nullptr, N, P1).bytes;
}

int32_t mr_icp_plane_iterate(const float* x, const float* y, const float* y_normals, int64_t N, int64_t P1, int64_t P2,
                             const int64_t* x_lengths, const int64_t* y_lengths, float max_dist2,
                             float relative_rmse_thr, int32_t max_iterations, int32_t iterations, float* rts,
                             float* history, float* rmse, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_icp_plane_iterate("icp plane", x, y, y_normals, N, P1, P2, max_dist2, max_iterations, iterations, rts,
                                       history, rmse, status, ws))
    return rc;
  const IcpPlaneWS w = carve_icp_plane(ws, N, P1);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "icp plane workspace too small");
  const NNGeom g = nn_geom(N, P1, P2, MRI_WANT_GROUPS);
  if (g.groups[0] > 0x7fffffffll) return set_err(MR_EUNSUPPORTED, "icp plane: P1 * P2 is too large for one launch");
  const hipStream_t st = (hipStream_t)stream;
  const ScanSearch search{x, y, g, x_lengths, y_lengths, rts, status, max_iterations, w.icp.key, st};
  return icp_plane_iterations(search, x, y, y_normals, N, P1, P2, x_lengths, y_lengths, max_dist2, relative_rmse_thr,
                              max_iterations, iterations, rts, history, rmse, status, w, st);
}

int32_t mr_icp_plane_iterate_grid(const float* x, const float* y, const float* y_normals, int64_t N, int64_t P1,
                                  int64_t P2, const int64_t* x_lengths, const int64_t* y_lengths, const void* grid,
                                  size_t grid_bytes, float max_dist2, float relative_rmse_thr, int32_t max_iterations,
                                  int32_t iterations, float* rts, float* history, float* rmse, int32_t* status,
                                  uint64_t* visited, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_icp_plane_iterate("icp plane grid", x, y, y_normals, N, P1, P2, max_dist2, max_iterations, iterations,
                                       rts, history, rmse, status, ws))
    return rc;
  GridBuf b;
  if (int rc = check_icp_grid("icp plane grid", grid, grid_bytes, N, P2, b)) return rc;
  const IcpPlaneWS w = carve_icp_plane(ws, N, P1);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "icp plane grid: icp plane workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  const GridSearch search{x, N, P1, P2, x_lengths, y_lengths, b, rts, max_dist2, status, max_iterations, w.icp.key,
                          (u64*)visited, st};
  return icp_plane_iterations(search, x, y, y_normals, N, P1, P2, x_lengths, y_lengths, max_dist2, relative_rmse_thr,
                              max_iterations, iterations, rts, history, rmse, status, w, st);
}

int32_t mr_icp_plane_solve_host(const double* A21, const double* b6, const float* rts_in, const double* c3,
                                float* rts_out) {
  if (!A21 || !b6 || !rts_in || !c3 || !rts_out) return set_err(MR_EINVAL, "icp plane solve: NULL pointer");
  const double c[3] = {c3[0], c3[1], c3[2]};
  plane_step(A21, b6, rts_in, c, rts_out);
  return MR_OK;
}

size_t mr_points_alignment_workspace(int64_t N, int64_t P) {
  if (!sizes_ok(N, P, P)) return 0;
  Carver c(nullptr);
  c.take<double>((size_t)(N * MRI_XC));
  c.take<double>((size_t)(N * ceil_div(P, MRR_TILE) * MRI_MOM));
  return c.off;
}

int32_t mr_points_alignment(const float* x, const float* y, int64_t N, int64_t P, const int64_t* lengths,
                            const float* weights, int32_t flags, double eps, float* rts, void* ws, size_t ws_bytes,
                            void* stream) {
  if (int rc = check_icp("points alignment", x, N, P, P)) return rc;
  if (flags & ~MR_ICP_ALL) return set_err(MR_EINVAL, "points alignment: unknown bits in flags");
  if (!(eps >= 0.0)) return set_err(MR_EINVAL, "points alignment: eps must be >= 0");
  if (!y || !rts || !ws) return set_err(MR_EINVAL, "points alignment: NULL pointer");
  if (ws_bytes < mr_points_alignment_workspace(N, P)) return set_err(MR_EWORKSPACE, "points alignment workspace too small");
  Carver c(ws);
  double* xc = c.take<double>((size_t)(N * MRI_XC));
  const int64_t nblk = ceil_div(P, MRR_TILE);
  double* mom = c.take<double>((size_t)(N * nblk * MRI_MOM));
  const hipStream_t st = (hipStream_t)stream;
  const dim3 gt((unsigned)nblk, (unsigned)N);
  const float* nof = nullptr;
  const int32_t* noi = nullptr;
  if (int rc = launch(KID_NONE, "k_icp_xstats", k_icp_xstats, (unsigned)N, MRR_BLOCK, 0, st, x, P, lengths, weights, eps, xc, nof,
                      nof, nof, (float*)nullptr))
    return rc;
  if (int rc = launch(KID_NONE, "k_icp_moments", k_icp_moments, gt, MRR_BLOCK, 0, st, x, y, P, P, lengths, lengths, weights,
                      (const double*)xc, noi, 0, (u64*)nullptr, (int32_t*)nullptr, mom, nblk))
    return rc;
  return launch(KID_NONE, "k_icp_solve", k_icp_solve, dim3(1, (unsigned)N), MRR_BLOCK, 0, st, x, y, N, P, P, lengths, weights,
                (const double*)xc, (const double*)mom, nblk, noi, flags, eps, noi, 0, rts, (float*)nullptr, (double*)nullptr);
}

}  // extern "C"
