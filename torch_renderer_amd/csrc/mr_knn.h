// mi355r — What the K-deep neighbour scans (mr_knn.hip's k_knn / k_knn_merge, mr_normals.hip's k_frames /
// k_frames_merge) share: the launch geometry with its split rule, the insertion into the register-resident ascending
// key list, and, as functions, the scan of a target range into the lists and the merge of a query's partial lists.
// k_knn and k_knn_merge keep these two loops written out: called as functions they compile to other code objects
// (profiles/normals_codeobj.txt), and their instantiations are measured as they are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mr_cloud.h"

#define MRK_MAXSPLIT 16
#define MRK_CUS 256            // fewer (cloud, query tile) pairs than this: the target range is split
#define MRK_WANT_GROUPS 1024   // workgroups a split launch aims for
#define MRK_SPLIT_ALIGN 64     // a split's targets are a multiple of this
#define MRK_TBLOCK 256         // threads of the per-query kernels

namespace {

struct KnnGeom {
  int kb, q;        // the bucket of K; queries per thread
  int64_t qtiles;   // query tiles per cloud
  int splits;
  int64_t per;      // targets per split
  int chunk;        // targets staged at a time
};

// The bucket is the power of two K rounds up to, at least min_kb.
inline KnnGeom knn_geom(int64_t N, int64_t P1, int64_t P2, int K, int min_kb = 1) {
  KnnGeom g;
  g.kb = min_kb;
  while (g.kb < K) g.kb *= 2;
  g.q = g.kb <= 8 ? 4 : (g.kb == 16 ? 2 : 1);
  g.qtiles = (P1 + MRN_BLOCK * g.q - 1) / (MRN_BLOCK * g.q);
  g.splits = 1;
  g.per = P2;
  const int64_t groups = N * g.qtiles;
  if (groups < MRK_CUS) {
    int64_t want = (MRK_WANT_GROUPS + groups - 1) / groups;
    if (want > MRK_MAXSPLIT) want = MRK_MAXSPLIT;
    g.per = ((P2 + want - 1) / want + MRK_SPLIT_ALIGN - 1) / MRK_SPLIT_ALIGN * MRK_SPLIT_ALIGN;
    g.splits = (int)((P2 + g.per - 1) / g.per);
  }
  g.chunk = (int)(g.per < MRN_MAXCHUNK ? g.per : MRN_MAXCHUNK);
  return g;
}

// The split launch's partial lists: (N, P1, splits, K) keys.
inline size_t knn_part_bytes(int64_t N, int64_t P1, int K, const KnnGeom& g) {
  return g.splits > 1 ? sizeof(u64) * (size_t)(N * P1) * (size_t)K * (size_t)g.splits : 0;
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
