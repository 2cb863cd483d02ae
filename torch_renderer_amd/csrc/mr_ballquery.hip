// mi355r — Radius neighbourhoods of point clouds (PyTorch3D ball_query): mr_ball_query / mr_ball_query_geometry /
// mr_ball_query_grid of include/mi355r.h. (mr_ball_query_backward is mr_knn.hip's neighbour_backward at norm 2.)
//
//   k_ball<Q, MODE>  a workgroup owns a tile of queries (Q per thread: mr_knn.h's scan_tile, the query load and the
//                    staging of mr_cloud.h's scan) and walks a range of its cloud's targets in ascending LDS chunks.
//                    A query keeps ONE register of state, the slots it has filled: a target with d < r2 is stored
//                    straight to slot (row * K + filled) of dists / idx, so K = 500 costs a candidate nothing. There
//                    is no list, no sort and no memset: every thread pads its own free slots with 0 / -1 when the
//                    walk is over.
//                    The result is the first K hits in index order, so a full query can stop: a wave tests, every
//                    MRB_STRIDE targets, with a ballot whether a lane still has a free slot and skips the rest of the
//                    chunk if none has (it still stages and meets every barrier), and the workgroup leaves the chunk
//                    loop through __syncthreads_or once both waves are full, never by a return before a barrier.
//   MODE 0           the whole cloud in one launch.
//   MODE 1 / MODE 2  when N * query tiles cannot fill the chip the target range is cut into <= 16 splits (ball_geom,
//                    from the shapes alone) and walked twice. The counting pass stores every (query, split)'s hits,
//                    capped at K: (N, splits, P1) int32 of workspace. The writing pass starts a split at the sum of
//                    the earlier splits' counts, rescans only while that is below K for some lane, and the last split
//                    pads. Index order is kept, so the result is bitwise that of MODE 0.
//   k_ball_query_grid<KB>  mr_ball_query_grid, K <= 64: one query per lane walks a point grid of the targets (mr_grid.h's
//                    grid_walk in its BALL form) and keeps its K lowest-indexed hits in registers: the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mi355r.h"
#include "mr_host.h"
#include "mr_cloud.h"
#include "mr_knn.h"
#include "mr_grid.h"

#define MRB_STRIDE 32  // targets between two tests of "is the wave full"
#define MRB_GRID_MAXK 64  // the deepest list k_ball_query_grid keeps

namespace {

// Q is the largest of 4, 2, 1 that still gives every compute unit two workgroups (else 1). Below one workgroup per
// unit, mr_knn.h's split rule with two settings of its own: only a cloud of more than two chunks is cut, into splits
// of at least one chunk. A shorter cloud is launch-bound either way, and the split path scans twice.
inline KnnGeom ball_geom(int64_t N, int64_t P1, int64_t P2) {
  KnnGeom g;
  g.kb = 0;
  g.q = 4;
  while (g.q > 1 && N * ((P1 + MRN_BLOCK * g.q - 1) / (MRN_BLOCK * g.q)) < 2 * MRK_CUS) g.q /= 2;
  knn_split(g, N, P1, P2, MRN_MAXCHUNK, false);
  return g;
}

template <int Q> __device__ __forceinline__ bool any_free(const int (&c)[Q], int K) {
  bool f = false;
#pragma unroll
  for (int k = 0; k < Q; ++k) f = f || c[k] < K;
  return f;
}

// grid (query tiles * splits, N). cnt: (N, splits, P1) hits per (query, split), written by MODE 1, read by MODE 2.
template <int Q, int MODE>
__global__ void __launch_bounds__(MRN_BLOCK) k_ball(const float* __restrict__ p1, const float* __restrict__ p2,
                                                    int64_t P1, int64_t P2, const int64_t* __restrict__ l1,
                                                    const int64_t* __restrict__ l2, float r2, int K, int splits,
                                                    int64_t per, float* __restrict__ dists, int32_t* __restrict__ idx,
                                                    int32_t* __restrict__ cnt) {
  __shared__ float4 sm[MRN_MAXCHUNK];
  // skip_outside is off: a tile outside its cloud starts with every c[k] = K, and `go` below ends it before a chunk
  const ScanTile tile = scan_tile<Q>(splits, per, l1, P1, l2, P2, false);
  const int64_t n = tile.n, q0 = tile.q0, lq = tile.lq, tb = tile.tb, te = tile.te;
  const int s = tile.s;
  const float* __restrict__ q = p1 + 3 * n * P1;
  const float* __restrict__ t = p2 + 3 * n * P2;

  float qx[Q], qy[Q], qz[Q];
  int c[Q];  // slots filled so far; K for a row that takes no hits
  scan_load_queries(q, q0, lq, nullptr, false, qx, qy, qz);
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    const int64_t i = q0 + k * MRN_BLOCK + threadIdx.x;
    int start = 0;
    if (MODE == 2 && i < lq) {
      const int32_t* __restrict__ pc = cnt + (n * splits) * P1 + i;
      for (int e = 0; e < s; ++e) start += pc[(int64_t)e * P1];  // each <= K and splits <= 16: no overflow
      if (start > K) start = K;
    }
    c[k] = i < lq ? start : K;
  }

  bool go = __syncthreads_or(any_free<Q>(c, K)) != 0;
  for (int64_t t0 = tb; go && t0 < te; t0 += MRN_MAXCHUNK) {  // `go` is uniform over the workgroup
    const int n_t = (int)((te - t0 < MRN_MAXCHUNK) ? te - t0 : MRN_MAXCHUNK);
    scan_stage(sm, t, t0, n_t, nullptr, false);
    __syncthreads();
    const int32_t base = (int32_t)t0;
    for (int j0 = 0; j0 < n_t; j0 += MRB_STRIDE) {
      if (!__any(any_free<Q>(c, K))) break;  // uniform over the wave: every lane of it is full
      const int je = j0 + MRB_STRIDE < n_t ? j0 + MRB_STRIDE : n_t;
#pragma unroll 2
      for (int j = j0; j < je; ++j) {
        const float4 p = sm[j];
#pragma unroll
        for (int k = 0; k < Q; ++k) {
          const float dd = dist3<2>(qx[k], qy[k], qz[k], p);
          if (dd < r2 && c[k] < K) {  // false for a nan distance
            if (MODE != 1) {
              const int64_t o = (n * P1 + q0 + k * MRN_BLOCK + threadIdx.x) * K + c[k];
              dists[o] = dd;
              idx[o] = base + j;
            }
            ++c[k];
          }
        }
      }
    }
    go = __syncthreads_or(any_free<Q>(c, K)) != 0;  // also: this chunk has been read
  }

#pragma unroll
  for (int k = 0; k < Q; ++k) {
    const int64_t i = q0 + k * MRN_BLOCK + threadIdx.x;
    if (i >= P1) continue;
    if (MODE == 1) {
      cnt[(n * splits + s) * P1 + i] = i < lq ? c[k] : 0;
    } else if (MODE == 0 || s == splits - 1) {  // the last split ends at the row's total
      const int64_t o = (n * P1 + i) * K;
      for (int e = i < lq ? c[k] : 0; e < K; ++e) {
        dists[o + e] = 0.0f;
        idx[o + e] = -1;
      }
    }
  }
}

// grid (blocks over P1, N), one wave a workgroup: mr_ball_query's result through a point grid of the targets
// (mr_grid.h). One query per lane; a hit (d < r2, strict) enters the lane's ascending list on ball_key, index first,
// so the list ends as the K lowest-indexed hits: the first K in index order. Candidates arrive in no index order and
// a full list stops nothing; the walk ends after ring r >= 1 once ring_bound(r) > r2 (every target beyond the rings
// is then at a distance >= the bound > r2 and cannot be a hit) or when the rings cover the grid.
template <int KB>
__global__ void __launch_bounds__(MRG_QBLOCK) k_ball_query_grid(const float* __restrict__ p1, int64_t P1, int64_t P2,
                                                                const int64_t* __restrict__ l1,
                                                                const int64_t* __restrict__ l2, int64_t budget,
                                                                const GridHead* __restrict__ heads,
                                                                const uint32_t* __restrict__ cell_start,
                                                                const float4* __restrict__ pts, float r2, int K,
                                                                float* __restrict__ dists, int32_t* __restrict__ idx,
                                                                u64* __restrict__ visited) {
  const int64_t n = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * MRG_QBLOCK + threadIdx.x;
  const int64_t lq = cloud_len(l1, n, P1);
  const uint32_t lt = (uint32_t)cloud_len(l2, n, P2);
  const GridHead H = heads[n];
  int gx, gy, gz;
  head_dims(H, budget, gx, gy, gz);
  u64 L[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) L[j] = ~0ull;
  uint32_t seen = 0u;
  if (i < lq && lt > 0u) {
    const float* __restrict__ q = p1 + 3 * (n * P1 + i);
    grid_walk<2, KB, true, true>(H, gx, gy, gz, cell_start + n * (budget + 1), pts + n * P2, lt, (uint32_t)(P2 - 1),
                                 q[0], q[1], q[2], K, r2, L, seen);
  }
  if (i < P1) {
    float* __restrict__ od = dists + (n * P1 + i) * K;
    int32_t* __restrict__ oi = idx + (n * P1 + i) * K;
#pragma unroll
    for (int s = 0; s < KB; ++s) {
      const bool ok = L[s] != ~0ull;  // a row past its length never walked
      if (s < K) {
        od[s] = ok ? __uint_as_float((uint32_t)L[s]) : 0.0f;
        oi[s] = ok ? (int32_t)(L[s] >> 32) : -1;
      }
    }
  }
  if (visited) grid_count_visited(seen, visited);
}

int check_ball(const char* who, const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2, float radius,
               int32_t K) {
  if (int rc = check_sizes(who, N, P1, P2)) return rc;
  if (K < 1) return set_err(MR_EINVAL, "%s: K must be >= 1", who);
  if (!(radius >= 0.0f) || __builtin_isinf(radius)) return set_err(MR_EINVAL, "%s: radius must be finite and >= 0", who);
  if (N * P1 >= (1ll << 62) / K) return set_err(MR_EUNSUPPORTED, "%s: N * P1 * K is too large", who);
  if (!p1 || !p2) return set_err(MR_EINVAL, "%s: p1 / p2 is NULL", who);
  return MR_OK;
}

}  // namespace

extern "C" {

int32_t mr_ball_query_geometry(int64_t N, int64_t P1, int64_t P2, int32_t K, int32_t* queries_per_group,
                               int32_t* splits, int32_t* lds_chunk) {
  if (N < 1 || P1 < 1 || P2 < 1 || K < 1)
    return set_err(MR_EINVAL, "ball query geometry: N, P1, P2 and K must be >= 1");
  if (int rc = check_sizes("ball query geometry", N, P1, P2)) return rc;
  geom_out(ball_geom(N, P1, P2), queries_per_group, splits, lds_chunk);
  return MR_OK;
}

size_t mr_ball_query_workspace(int64_t N, int64_t P1, int64_t P2, int32_t K) {
  if (!sizes_ok(N, P1, P2) || K < 1) return 0;
  const KnnGeom g = ball_geom(N, P1, P2);
  Carver c(nullptr);
  c.take<int32_t>((g.splits > 1 ? (size_t)(N * P1) * (size_t)g.splits : 0) + 1);  // never 0: 0 means out of range
  return c.off;
}

int32_t mr_ball_query(const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2, const int64_t* lengths1,
                      const int64_t* lengths2, float radius, int32_t K, float* dists, int32_t* idx, void* ws,
                      size_t ws_bytes, void* stream) {
  if (int rc = check_ball("ball query", p1, p2, N, P1, P2, radius, K)) return rc;
  if (!dists || !idx || !ws) return set_err(MR_EINVAL, "ball query: dists / idx / workspace is NULL");
  if (ws_bytes < mr_ball_query_workspace(N, P1, P2, K)) return set_err(MR_EWORKSPACE, "ball query workspace too small");
  const KnnGeom g = ball_geom(N, P1, P2);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(g.qtiles * g.splits), (unsigned)N);
  const float r2 = radius * radius;
  const int k = K, splits = g.splits;
  int32_t* cnt = g.splits > 1 ? (int32_t*)ws : nullptr;
#define MRB_SCAN(Q, MODE)                                                                                            \
  launch(KID_NONE, "k_ball", k_ball<Q, MODE>, grid, MRN_BLOCK, 0, st, p1, p2, P1, P2, lengths1, lengths2, r2, k, splits, \
         g.per, dists, idx, cnt)
#define MRB_SCAN_Q(MODE) (g.q == 4 ? MRB_SCAN(4, MODE) : (g.q == 2 ? MRB_SCAN(2, MODE) : MRB_SCAN(1, MODE)))
  if (!cnt) return MRB_SCAN_Q(0);
  if (int rc = MRB_SCAN_Q(1)) return rc;
  return MRB_SCAN_Q(2);
#undef MRB_SCAN_Q
#undef MRB_SCAN
}

size_t mr_ball_query_grid_workspace(int64_t N, int64_t P1, int64_t P2, int32_t K) {
  if (!sizes_ok(N, P1, P2) || K < 1 || K > MRB_GRID_MAXK) return 0;
  return 256;  // nothing is kept between the lanes; never 0, which means "out of range"
}

int32_t mr_ball_query_grid(const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2, const int64_t* lengths1,
                           const int64_t* lengths2, const void* grid, size_t grid_bytes, float radius, int32_t K,
                           float* dists, int32_t* idx, uint64_t* visited, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_ball("ball query grid", p1, p2, N, P1, P2, radius, K)) return rc;
  if (K > MRB_GRID_MAXK) return set_err(MR_EUNSUPPORTED, "ball query grid: K > %d is not built", MRB_GRID_MAXK);
  if (!dists || !idx || !ws || !grid)
    return set_err(MR_EINVAL, "ball query grid: dists / idx / grid / workspace is NULL");
  const GridBuf b = carve_grid(grid, N, P2);
  if (grid_bytes < b.bytes) return set_err(MR_EWORKSPACE, "ball query grid: grid buffer too small");
  if (ws_bytes < mr_ball_query_grid_workspace(N, P1, P2, K))
    return set_err(MR_EWORKSPACE, "ball query grid workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  const int64_t budget = grid_budget(P2);
  const dim3 g((unsigned)ceil_div(P1, MRG_QBLOCK), (unsigned)N);
  const float r2 = radius * radius;
  const int k = K;
  int kb = 1;
  while (kb < K) kb *= 2;
#define MRB_GRID(KB)                                                                                              \
  case KB:                                                                                                        \
    return launch(KID_NONE, "k_ball_query_grid", k_ball_query_grid<KB>, g, MRG_QBLOCK, 0, st, p1, P1, P2, lengths1, \
                  lengths2, budget, (const GridHead*)b.head, (const uint32_t*)b.cell_start, (const float4*)b.pts, r2, \
                  k, dists, idx, (u64*)visited)
  switch (kb) {
    MRB_GRID(1);
    MRB_GRID(2);
    MRB_GRID(4);
    MRB_GRID(8);
    MRB_GRID(16);
    MRB_GRID(32);
    default:
      MRB_GRID(64);
  }
#undef MRB_GRID
}

}  // extern "C"
