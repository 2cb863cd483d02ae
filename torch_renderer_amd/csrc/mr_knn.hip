// mi355r — K nearest neighbours of point clouds (PyTorch3D knn_points, 1 <= K <= 32) and the gradient of their
// distances: mr_knn_points / mr_knn_points_backward / mr_knn_geometry of include/mi355r.h.
//
//   k_knn         a workgroup owns a tile of queries (Q per thread) and scans a range of its cloud's targets itself
//                 (mr_knn.h's scan_tile and knn_scan over the query load and the staging of mr_cloud.h's scan). Every
//                 query keeps its KB smallest keys (nn_key) ascending in registers: KB is the compile-time bucket (1, 2,
//                 4, 8, 16, 32) the requested K rounds up to, and Q = 4, 4, 4, 4, 2, 1 keeps the lists at <= 64 VGPRs.
//                 A candidate costs one compare, its distance bits against those of the worst kept key (targets arrive
//                 in ascending index order, so an equal distance never displaces a kept key: ties go to the lowest
//                 index); only a smaller one runs the unrolled insertion. With splits == 1 the range is the whole
//                 cloud and the workgroup writes dists / idx itself (knn_store): no key buffer, memset, atomic or
//                 merge. Only when N * query tiles < 256 (the CUs) is the target range cut into <= 16 splits, from the
//                 shapes alone; a workgroup then writes its K sorted keys per query into the workspace (8 K splits
//                 bytes per query) and
//   k_knn_merge   (one thread per query) merges a query's partial lists by key (knn_merge_lists) and decodes.
//                 The key order is total, so the K kept do not depend on the splits or the chunk size.
// The backward, neighbour_backward, is three launches and no memset, for mr_knn_points_backward and, at any K and
// norm 2, for mr_ball_query_backward:
//   k_zero_words  clears the fixed-point rows;
//   k_knn_bwd     one thread per query: grad_p1 = sum_k 2 g (p1 - p2[idx]) (norm 1: g sign(.)) with a plain store, and
//                 the same addends into the targets' rows with 64-bit fixed-point integer atomics (mr_common.h);
//   k_knn_bwd_p2  grad_p2 = -(row). Slots with idx < 0 contribute nothing and their g is not read.
// The geometry (knn_geom), the split constants, the list code with its decoding store (knn_store) and the argument
// check (check_knn) are mr_knn.h's, shared with mr_normals.hip, mr_ballquery.hip and mr_grid.hip. The two bucket
// ladders below stay macros of this file: mr_normals.hip's run over other buckets (8 .. 64) with other arguments, and
// one dispatcher for both would need the kernel as a template template argument.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mi355r.h"
#include "mr_common.h"
#include "mr_host.h"
#include "mr_cloud.h"
#include "mr_knn.h"

namespace {

// grid (query tiles * splits, N). part != NULL: (N, P1, splits, K) keys; else dists / idx (N, P1, K).
template <int NORM, int KB, int Q>
__global__ void __launch_bounds__(MRN_BLOCK) k_knn(const float* __restrict__ p1, const float* __restrict__ p2, int64_t P1,
                                                   int64_t P2, const int64_t* __restrict__ l1,
                                                   const int64_t* __restrict__ l2, int K, int splits, int64_t per,
                                                   float* __restrict__ dists, int32_t* __restrict__ idx,
                                                   u64* __restrict__ part) {
  __shared__ float4 sm[MRN_MAXCHUNK];
  const ScanTile c = scan_tile<Q>(splits, per, l1, P1, l2, P2, true);
  float qx[Q], qy[Q], qz[Q];
  u64 L[Q][KB];
  scan_load_queries(p1 + 3 * c.n * P1, c.q0, c.lq, nullptr, false, qx, qy, qz);
#pragma unroll
  for (int k = 0; k < Q; ++k)
#pragma unroll
    for (int j = 0; j < KB; ++j) L[k][j] = ~0ull;
  knn_scan<NORM, KB, Q>(sm, p2 + 3 * c.n * P2, c.tb, c.te, qx, qy, qz, L);
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    const int64_t i = c.q0 + k * MRN_BLOCK + threadIdx.x;
    if (i >= P1) continue;
    const int64_t row = c.n * P1 + i;
    if (part) {
      knn_store_keys<KB>(L[k], i < c.lq, K, part + (row * splits + c.s) * K);
    } else {
      knn_store<KB>(L[k], i < c.lq, K, dists + row * K, idx + row * K);
    }
  }
}

// One thread per row of (N, P1): its `splits` ascending lists of K keys -> the K smallest, decoded.
template <int KB>
__global__ void __launch_bounds__(MRK_TBLOCK) k_knn_merge(const u64* __restrict__ part, int64_t rows, int K, int splits,
                                                          float* __restrict__ dists, int32_t* __restrict__ idx) {
  const int64_t row = (int64_t)blockIdx.x * MRK_TBLOCK + threadIdx.x;
  if (row >= rows) return;
  u64 L[KB];
  knn_merge_lists<KB>(part, row, K, splits, L);
  knn_store<KB>(L, true, K, dists + row * K, idx + row * K);
}

// grid (blocks over P1, N). fix / rem: (N, P2, 3) rows of the targets.
template <int NORM>
__global__ void __launch_bounds__(MRK_TBLOCK) k_knn_bwd(const float* __restrict__ p1, const float* __restrict__ p2,
                                                        int64_t P1, int64_t P2, const int64_t* __restrict__ l1,
                                                        const int64_t* __restrict__ l2, int K,
                                                        const int32_t* __restrict__ idx, const float* __restrict__ g,
                                                        float* __restrict__ grad_p1, u64* __restrict__ fix,
                                                        float* __restrict__ rem) {
  const int64_t n = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * MRK_TBLOCK + threadIdx.x;
  if (i >= P1) return;
  const int64_t row = n * P1 + i;
  const int64_t lt = cloud_len(l2, n, P2);
  const float* __restrict__ q = p1 + 3 * row;
  float acc[3] = {0.0f, 0.0f, 0.0f};
  if (i < cloud_len(l1, n, P1)) {
    const float q0 = q[0], q1 = q[1], q2 = q[2];
    for (int k = 0; k < K; ++k) {
      const int32_t j = idx[row * K + k];
      if (j < 0 || j >= lt) continue;
      const float up = g[row * K + k];
      const float* __restrict__ t = p2 + 3 * (n * P2 + j);
      const float df[3] = {q0 - t[0], q1 - t[1], q2 - t[2]};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = NORM == 2 ? (2.0f * up) * df[c] : up * sgn(df[c]);
        acc[c] += v;
        fix_add(fix, rem, 3 * (n * P2 + j) + c, v);
      }
    }
  }
  grad_p1[3 * row] = acc[0];
  grad_p1[3 * row + 1] = acc[1];
  grad_p1[3 * row + 2] = acc[2];
}

__global__ void __launch_bounds__(MRK_TBLOCK) k_knn_bwd_p2(const u64* __restrict__ fix, const float* __restrict__ rem,
                                                           int64_t n, float* __restrict__ grad_p2) {
  const int64_t i = (int64_t)blockIdx.x * MRK_TBLOCK + threadIdx.x;
  if (i < n) grad_p2[i] = 0.0f - fix_read(fix, rem, i);  // +0 for a target nothing reached
}

__global__ void __launch_bounds__(MRK_TBLOCK) k_zero_words(u64* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * MRK_TBLOCK + threadIdx.x;
  if (i < n) p[i] = 0ull;
}

// The gradient of a neighbour search's dists behind mr_knn_points_backward and mr_ball_query_backward, whose own
// checks of the sizes, K and norm have passed: k_zero_words clears the fixed-point rows, then the two kernels above.
// A kernel clears them, not a memset: in a captured graph of forward + backward a memset node cleared them on the
// first replay only (tests/test_gpu_knn.py and test_gpu_ball_query.py replay twice with changed inputs).
size_t neighbour_backward_workspace(int64_t N, int64_t P1, int64_t P2, int32_t K, int32_t max_k) {
  if (!sizes_ok(N, P1, P2) || K < 1 || K > max_k) return 0;
  return carve_fix(nullptr, 3 * N * P2).bytes;
}

int neighbour_backward(const char* who, int32_t norm, int32_t K, const float* p1, const float* p2, int64_t N,
                       int64_t P1, int64_t P2, const int64_t* lengths1, const int64_t* lengths2, const int32_t* idx,
                       const float* grad_dists, float* grad_p1, float* grad_p2, void* ws, size_t ws_bytes,
                       void* stream) {
  if (!p1 || !p2 || !idx || !grad_dists || !grad_p1 || !grad_p2 || !ws)
    return set_err(MR_EINVAL, "%s: NULL pointer", who);
  const FixWS w = carve_fix(ws, 3 * N * P2);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "%s workspace too small", who);
  const hipStream_t st = (hipStream_t)stream;
  const int64_t words = (int64_t)(w.bytes / sizeof(u64));  // the carve ends on a multiple of 256 B
  if (int rc = launch(KID_NONE, "k_zero_words", k_zero_words, (unsigned)ceil_div(words, MRK_TBLOCK), MRK_TBLOCK, 0, st,
                      (u64*)ws, words))
    return rc;
  const dim3 grid((unsigned)ceil_div(P1, MRK_TBLOCK), (unsigned)N);
  const int k = K;
  if (int rc = launch(KID_NONE, "k_knn_bwd", norm == 2 ? k_knn_bwd<2> : k_knn_bwd<1>, grid, MRK_TBLOCK, 0, st, p1, p2, P1, P2,
                      lengths1, lengths2, k, idx, grad_dists, grad_p1, w.fix, w.rem))
    return rc;
  return launch(KID_NONE, "k_knn_bwd_p2", k_knn_bwd_p2, (unsigned)ceil_div(3 * N * P2, MRK_TBLOCK), MRK_TBLOCK, 0, st,
                (const u64*)w.fix, (const float*)w.rem, 3 * N * P2, grad_p2);
}

}  // namespace

extern "C" {

int32_t mr_knn_geometry(int64_t N, int64_t P1, int64_t P2, int32_t K, int32_t* queries_per_group, int32_t* splits,
                        int32_t* lds_chunk) {
  if (N < 1 || P1 < 1 || P2 < 1 || K < 1) return set_err(MR_EINVAL, "knn geometry: N, P1, P2 and K must be >= 1");
  if (K > MRK_MAXK) return set_err(MR_EUNSUPPORTED, "knn geometry: K > %d is not built", MRK_MAXK);
  if (int rc = check_sizes("knn geometry", N, P1, P2)) return rc;
  geom_out(knn_geom(N, P1, P2, K), queries_per_group, splits, lds_chunk);
  return MR_OK;
}

size_t mr_knn_points_workspace(int64_t N, int64_t P1, int64_t P2, int32_t K) {
  if (!sizes_ok(N, P1, P2) || K < 1 || K > MRK_MAXK) return 0;
  return knn_ws_bytes(N, P1, K, knn_geom(N, P1, P2, K));
}

int32_t mr_knn_points(const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2, const int64_t* lengths1,
                      const int64_t* lengths2, int32_t norm, int32_t K, float* dists, int32_t* idx, void* ws,
                      size_t ws_bytes, void* stream) {
  if (int rc = check_knn("knn points", p1, p2, N, P1, P2, norm, K)) return rc;
  if (!dists || !idx || !ws) return set_err(MR_EINVAL, "knn points: dists / idx / workspace is NULL");
  if (ws_bytes < mr_knn_points_workspace(N, P1, P2, K)) return set_err(MR_EWORKSPACE, "knn points workspace too small");
  const KnnGeom g = knn_geom(N, P1, P2, K);
  const hipStream_t st = (hipStream_t)stream;
  u64* part = g.splits > 1 ? (u64*)ws : nullptr;
  const dim3 grid((unsigned)(g.qtiles * g.splits), (unsigned)N);
  const int k = K, splits = g.splits;
  int rc;
#define MRK_SCAN(NORM, KB, Q)                                                                                         \
  rc = launch(KID_NONE, "k_knn", k_knn<NORM, KB, Q>, grid, MRN_BLOCK, 0, st, p1, p2, P1, P2, lengths1, lengths2, k, splits, \
              g.per, dists, idx, part)
#define MRK_SCAN_K(NORM)            \
  switch (g.kb) {                   \
    case 1: MRK_SCAN(NORM, 1, 4); break;   \
    case 2: MRK_SCAN(NORM, 2, 4); break;   \
    case 4: MRK_SCAN(NORM, 4, 4); break;   \
    case 8: MRK_SCAN(NORM, 8, 4); break;   \
    case 16: MRK_SCAN(NORM, 16, 2); break; \
    default: MRK_SCAN(NORM, 32, 1); break; \
  }
  if (norm == 2) {
    MRK_SCAN_K(2)
  } else {
    MRK_SCAN_K(1)
  }
#undef MRK_SCAN_K
#undef MRK_SCAN
  if (rc || !part) return rc;
  const int64_t rows = N * P1;
  const unsigned mg = (unsigned)((rows + MRK_TBLOCK - 1) / MRK_TBLOCK);
#define MRK_MERGE(KB)                                                                                            \
  case KB:                                                                                                       \
    return launch(KID_NONE, "k_knn_merge", k_knn_merge<KB>, mg, MRK_TBLOCK, 0, st, (const u64*)part, rows, k, splits, dists, \
                  idx)
  switch (g.kb) {
    MRK_MERGE(1);
    MRK_MERGE(2);
    MRK_MERGE(4);
    MRK_MERGE(8);
    MRK_MERGE(16);
    default:
    MRK_MERGE(32);
  }
#undef MRK_MERGE
}

size_t mr_knn_points_backward_workspace(int64_t N, int64_t P1, int64_t P2, int32_t K) {
  return neighbour_backward_workspace(N, P1, P2, K, MRK_MAXK);
}

int32_t mr_knn_points_backward(const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2,
                               const int64_t* lengths1, const int64_t* lengths2, int32_t norm, int32_t K,
                               const int32_t* idx, const float* grad_dists, float* grad_p1, float* grad_p2, void* ws,
                               size_t ws_bytes, void* stream) {
  if (int rc = check_knn("knn points backward", p1, p2, N, P1, P2, norm, K)) return rc;
  return neighbour_backward("knn points backward", norm, K, p1, p2, N, P1, P2, lengths1, lengths2, idx, grad_dists,
                            grad_p1, grad_p2, ws, ws_bytes, stream);
}

// The gradient of mr_ball_query's dists (mr_ballquery.hip): squared distances, at any K >= 1.
size_t mr_ball_query_backward_workspace(int64_t N, int64_t P1, int64_t P2, int32_t K) {
  return neighbour_backward_workspace(N, P1, P2, K, INT32_MAX);
}

int32_t mr_ball_query_backward(const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2,
                               const int64_t* lengths1, const int64_t* lengths2, int32_t K, const int32_t* idx,
                               const float* grad_dists, float* grad_p1, float* grad_p2, void* ws, size_t ws_bytes,
                               void* stream) {
  if (int rc = check_sizes("ball query backward", N, P1, P2)) return rc;
  if (K < 1) return set_err(MR_EINVAL, "ball query backward: K must be >= 1");
  return neighbour_backward("ball query backward", 2, K, p1, p2, N, P1, P2, lengths1, lengths2, idx, grad_dists,
                            grad_p1, grad_p2, ws, ws_bytes, stream);
}

}  // extern "C"
