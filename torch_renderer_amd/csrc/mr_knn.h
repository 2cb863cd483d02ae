// mi355r — What the neighbour scans (mr_knn.hip's k_knn / k_knn_merge, mr_normals.hip's k_frames / k_frames_merge,
// mr_ballquery.hip's k_ball) share, one copy of each. Host: the launch geometry (KnnGeom) with its split rule. Device:
// the workgroup's tile of queries and range of targets (scan_tile); for the K-deep lists, the insertion into the
// register-resident ascending key list, the scan of a target range into the lists, the store of a partial list and
// the merge of a query's partial lists. (k_frames keeps its own tile prologue and key store: mr_normals.hip says why.)
// mr_grid.hip's k_knn_grid takes the insertion, the decoding store (knn_store) and the argument check (check_knn).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mr_cloud.h"

#define MRK_MAXSPLIT 16
#define MRK_CUS 256            // fewer (cloud, query tile) pairs than this: the target range is split
#define MRK_WANT_GROUPS 1024   // workgroups a split launch aims for
#define MRK_SPLIT_ALIGN 64     // a split's targets are a multiple of this
#define MRK_TBLOCK 256         // threads of the per-query kernels
#define MRK_MAXK 32            // the deepest list mr_knn_points and mr_knn_points_grid keep

namespace {

struct KnnGeom {
  int kb, q;        // the bucket of K (0: no list is kept); queries per thread
  int64_t qtiles;   // query tiles per cloud
  int splits;
  int64_t per;      // targets per split
  int chunk;        // targets staged at a time
};

// The split rule, from g.q and the shapes alone: fewer (cloud, query tile) pairs than compute units cut the target
// range into <= MRK_MAXSPLIT splits of at least min_per targets, a multiple of MRK_SPLIT_ALIGN each. split_short:
// whether a cloud of at most two chunks is split at all.
inline void knn_split(KnnGeom& g, int64_t N, int64_t P1, int64_t P2, int64_t min_per, bool split_short) {
  g.qtiles = (P1 + MRN_BLOCK * g.q - 1) / (MRN_BLOCK * g.q);
  g.splits = 1;
  g.per = P2;
  const int64_t groups = N * g.qtiles;
  if (groups < MRK_CUS && (split_short || P2 > 2 * MRN_MAXCHUNK)) {
    int64_t want = (MRK_WANT_GROUPS + groups - 1) / groups;
    if (want > MRK_MAXSPLIT) want = MRK_MAXSPLIT;
    int64_t per = (P2 + want - 1) / want;
    if (per < min_per) per = min_per;
    g.per = (per + MRK_SPLIT_ALIGN - 1) / MRK_SPLIT_ALIGN * MRK_SPLIT_ALIGN;
    g.splits = (int)((P2 + g.per - 1) / g.per);
  }
  g.chunk = (int)(g.per < MRN_MAXCHUNK ? g.per : MRN_MAXCHUNK);
}

// The bucket is the power of two K rounds up to, at least min_kb.
inline KnnGeom knn_geom(int64_t N, int64_t P1, int64_t P2, int K, int min_kb = 1) {
  KnnGeom g;
  g.kb = min_kb;
  while (g.kb < K) g.kb *= 2;
  g.q = g.kb <= 8 ? 4 : (g.kb == 16 ? 2 : 1);
  knn_split(g, N, P1, P2, 1, true);
  return g;
}

// What the three *_geometry entry points report of a launch.
inline void geom_out(const KnnGeom& g, int32_t* queries_per_group, int32_t* splits, int32_t* lds_chunk) {
  if (queries_per_group) *queries_per_group = MRN_BLOCK * g.q;
  if (splits) *splits = g.splits;
  if (lds_chunk) *lds_chunk = g.chunk;
}

// The workspace of a K-deep scan: the split launch's partial lists, (N, P1, splits, K) keys. Never 0, which means
// "out of range" to the callers of the *_workspace entry points.
inline size_t knn_ws_bytes(int64_t N, int64_t P1, int K, const KnnGeom& g) {
  Carver c(nullptr);
  c.take<u64>((g.splits > 1 ? (size_t)(N * P1) * (size_t)K * (size_t)g.splits : 0) + 1);
  return c.off;
}

// What mr_knn_points, its backward and mr_knn_points_grid check first.
inline int check_knn(const char* who, const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2, int32_t norm,
                     int32_t K) {
  if (int rc = check_sizes(who, N, P1, P2)) return rc;
  if (K < 1) return set_err(MR_EINVAL, "%s: K must be >= 1", who);
  if (K > MRK_MAXK) return set_err(MR_EUNSUPPORTED, "%s: K > %d is not built", who, MRK_MAXK);
  if (norm != 1 && norm != 2) return set_err(MR_EINVAL, "%s: norm must be 1 or 2", who);
  if (!p1 || !p2) return set_err(MR_EINVAL, "%s: p1 / p2 is NULL", who);
  return MR_OK;
}

// A scanning workgroup's share of grid (query tiles * splits, N): cloud n, queries from q0 of its lq, and targets
// tb .. te of its lt, the split s. skip_outside: a tile with no query inside its cloud (uniform) scans nothing.
struct ScanTile {
  int64_t n, q0, lq, lt, tb, te;
  int s;
};
template <int Q>
__device__ __forceinline__ ScanTile scan_tile(int splits, int64_t per, const int64_t* l1, int64_t P1,
                                              const int64_t* l2, int64_t P2, bool skip_outside) {
  ScanTile c;
  c.n = blockIdx.y;
  c.q0 = ((int64_t)blockIdx.x / splits) * (MRN_BLOCK * Q);
  c.s = (int)((int64_t)blockIdx.x % splits);
  c.lq = cloud_len(l1, c.n, P1);
  c.lt = cloud_len(l2, c.n, P2);
  c.tb = (int64_t)c.s * per;
  c.te = c.tb + per < c.lt ? c.tb + per : c.lt;
  if (skip_outside && c.q0 >= c.lq) c.te = c.tb;
  return c;
}

// c < L[KB - 1] is known: c takes its place in the ascending list and the worst key leaves. Compile-time indices only.
template <int KB> __device__ __forceinline__ void knn_insert(u64 (&L)[KB], u64 c) {
#pragma unroll
  for (int i = KB - 1; i > 0; --i) {
    const u64 below = L[i - 1];
    L[i] = c < below ? below : (c < L[i] ? c : L[i]);
  }
  L[0] = c < L[0] ? c : L[0];
}

// Targets tb .. te of t (ascending, staged through sm in chunks) against Q queries: every list keeps its KB smallest
// keys. A candidate costs one compare, its distance bits against those of the worst kept key; targets arrive in
// ascending index order, so an equal distance never displaces a kept key. All threads of the workgroup call it.
template <int NORM, int KB, int Q>
__device__ __forceinline__ void knn_scan(float4* __restrict__ sm, const float* __restrict__ t, int64_t tb, int64_t te,
                                         const float (&qx)[Q], const float (&qy)[Q], const float (&qz)[Q],
                                         u64 (&L)[Q][KB]) {
  for (int64_t t0 = tb; t0 < te; t0 += MRN_MAXCHUNK) {
    const int cnt = (int)((te - t0 < MRN_MAXCHUNK) ? te - t0 : MRN_MAXCHUNK);
    if (t0 != tb) __syncthreads();  // the previous chunk has been read
    scan_stage(sm, t, t0, cnt, nullptr, false);
    __syncthreads();
    const uint32_t base = (uint32_t)t0;
#pragma unroll 2
    for (int j = 0; j < cnt; ++j) {
      const float4 p = sm[j];
#pragma unroll
      for (int k = 0; k < Q; ++k) {
        const float dd = dist3<NORM>(qx[k], qy[k], qz[k], p);
        if (__float_as_uint(dd) < key_bits(L[k][KB - 1])) knn_insert<KB>(L[k], nn_key(dd, base + (uint32_t)j));
      }
    }
  }
}

// The first K keys of a list into its place o of the partial lists; all-ones for a row past its length.
template <int KB>
__device__ __forceinline__ void knn_store_keys(const u64 (&L)[KB], bool row_ok, int K, u64* o) {
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    if (j < K) o[j] = row_ok ? L[j] : ~0ull;
  }
}

// The first K slots of a list as dists / idx: 0 / -1 for a slot that was never filled (or a row past its length).
template <int KB>
__device__ __forceinline__ void knn_store(const u64 (&L)[KB], bool row_ok, int K, float* __restrict__ od,
                                          int32_t* __restrict__ oi) {
#pragma unroll
  for (int s = 0; s < KB; ++s) {
    const bool ok = row_ok && L[s] != ~0ull;
    if (s < K) {
      od[s] = ok ? key_dist(L[s]) : 0.0f;
      oi[s] = ok ? (int32_t)key_index(L[s]) : -1;
    }
  }
}

// A row's `splits` ascending lists of K keys -> the K smallest in L (all-ones where fewer exist). A list's remaining
// keys are skipped at its first key that does not enter.
template <int KB>
__device__ __forceinline__ void knn_merge_lists(const u64* __restrict__ part, int64_t row, int K, int splits,
                                                u64 (&L)[KB]) {
#pragma unroll
  for (int j = 0; j < KB; ++j) L[j] = ~0ull;
  for (int s = 0; s < splits; ++s) {
    const u64* __restrict__ p = part + (row * splits + s) * K;
    for (int j = 0; j < K; ++j) {
      const u64 c = p[j];
      if (!(c < L[KB - 1])) break;
      knn_insert<KB>(L, c);
    }
  }
}

}  // namespace
