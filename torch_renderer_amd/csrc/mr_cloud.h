// mi355r — What the point-cloud translation units (mr_points.hip, mr_knn.hip, mr_normals.hip, mr_fps.hip,
// mr_pointmesh.hip, mr_ballquery.hip) share: the
// size limits and their host check, the clamped cloud length, the float32 distance with its fixed operation order, the
// packed (distance, index) key, the fixed-point rows of a scatter's targets, and the brute-force nearest-point scan
// (query load, target staging, compare loop) that k_nn, k_icp_nn, k_posed_nn, k_knn, k_frames and k_ball are built from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mr_host.h"

#define MRN_BLOCK 128       // threads of a scanning workgroup (two waves)
#define MRN_MAXCHUNK 1024   // targets staged at a time (16 KiB of LDS)

namespace {

typedef unsigned long long u64;

inline bool sizes_ok(int64_t N, int64_t P1, int64_t P2) {
  // per-cloud indices are int32; the grid's y dimension is the batch
  return N >= 1 && P1 >= 1 && P2 >= 1 && N <= 65535 && P1 < 0x7fffffffll && P2 < 0x7fffffffll &&
         N * P1 < (1ll << 40) / 3 && N * P2 < (1ll << 40) / 3;
}

// What every entry point over a batch of cloud pairs checks first.
inline int check_sizes(const char* who, int64_t N, int64_t P1, int64_t P2) {
  if (N < 1 || P1 < 1 || P2 < 1) return set_err(MR_EINVAL, "%s: N, P1 and P2 must be >= 1", who);
  if (!sizes_ok(N, P1, P2))
    return set_err(MR_EUNSUPPORTED, "%s: more than 65535 clouds or clouds too large for 32-bit point ids", who);
  return MR_OK;
}

// Fixed-point rows of a scatter's targets: `n` 64-bit words, then `n` float remainders.
struct FixWS {
  u64* fix;
  float* rem;
  size_t bytes;
};
inline FixWS carve_fix(void* base, int64_t n) {
  FixWS w;
  Carver c(base);
  w.fix = c.take_packed<u64>((size_t)n);  // words and remainders back to back: one memset
  w.rem = c.take<float>((size_t)n);
  w.bytes = c.off;
  return w;
}

__device__ __forceinline__ int64_t cloud_len(const int64_t* __restrict__ lengths, int64_t n, int64_t P) {
  if (!lengths) return P;
  const int64_t l = lengths[n];
  return l < 0 ? 0 : (l > P ? P : l);
}

template <int NORM> __device__ __forceinline__ float dist3(float qx, float qy, float qz, float4 t) {
  const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
  if (NORM == 2) return (dx * dx + dy * dy) + dz * dz;
  return (fabsf(dx) + fabsf(dy)) + fabsf(dz);
}

__device__ __forceinline__ float sgn(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }

// A candidate as one 64-bit word, (float bits of dist) << 32 | index. A distance is >= +0, and non-negative float
// bits order as unsigned integers: the smaller key is the nearer candidate and, at equal distances, the lower index,
// whatever order candidates arrive in (a 64-bit atomicMin merges them). All-ones (a memset of 0xff) is above every
// key: an empty slot.
__device__ __forceinline__ u64 nn_key(float dist, uint32_t index) {
  return ((u64)__float_as_uint(dist) << 32) | (u64)index;
}
__device__ __forceinline__ uint32_t key_bits(u64 key) { return (uint32_t)(key >> 32); }  // of the distance
__device__ __forceinline__ float key_dist(u64 key) { return __uint_as_float(key_bits(key)); }
__device__ __forceinline__ uint32_t key_index(u64 key) { return (uint32_t)key; }

// A cloud's transform is 13 floats, R (3x3 row-major), T (3), s: y = s (x R) + T with row vectors. The one transform
// code: the searches, the residual and the final points all call it.
__device__ __forceinline__ void sim_apply(const float* __restrict__ t, float x0, float x1, float x2, float& o0,
                                          float& o1, float& o2) {
  const float s = t[12];
  o0 = s * ((x0 * t[0] + x1 * t[3]) + x2 * t[6]) + t[9];
  o1 = s * ((x0 * t[1] + x1 * t[4]) + x2 * t[7]) + t[10];
  o2 = s * ((x0 * t[2] + x1 * t[5]) + x2 * t[8]) + t[11];
}

// ---------------------------------------------------------------------------
// The brute-force scan of a workgroup of MRN_BLOCK threads: Q queries per thread in registers, targets staged in LDS
// as float4 and read as a broadcast (every lane reads the same address; one read feeds Q distance evaluations).
// `apply` passes a point through the transform `tr` first (tr is not read otherwise).
// ---------------------------------------------------------------------------

// Queries q0 + k * MRN_BLOCK + threadIdx.x of a cloud of lq points; zeros past the length.
template <int Q>
__device__ __forceinline__ void scan_load_queries(const float* __restrict__ q, int64_t q0, int64_t lq,
                                                  const float* __restrict__ tr, bool apply, float (&qx)[Q],
                                                  float (&qy)[Q], float (&qz)[Q]) {
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    const int64_t i = q0 + k * MRN_BLOCK + threadIdx.x;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    if (i < lq) {  // one branch around the three loads
      a0 = q[3 * i];
      a1 = q[3 * i + 1];
      a2 = q[3 * i + 2];
    }
    if (apply) sim_apply(tr, a0, a1, a2, a0, a1, a2);
    qx[k] = a0;
    qy[k] = a1;
    qz[k] = a2;
  }
}

// Targets t0 .. t0 + cnt of t into sm[0 .. cnt). The caller synchronises (before, if sm is still being read, and after).
__device__ __forceinline__ void scan_stage(float4* __restrict__ sm, const float* __restrict__ t, int64_t t0, int cnt,
                                           const float* __restrict__ tr, bool apply) {
  for (int j = threadIdx.x; j < cnt; j += MRN_BLOCK) {
    const float* p = t + 3 * (t0 + j);
    float p0 = p[0], p1 = p[1], p2 = p[2];
    if (apply) sim_apply(tr, p0, p1, p2, p0, p1, p2);
    sm[j] = make_float4(p0, p1, p2, 0.0f);
  }
}

// The staged chunk against Q queries: best / bi keep the smallest distance and base + its place in the chunk. The
// comparison is strict, so inside a chunk, and across chunks scanned in ascending order, the lowest index wins a tie.
// The loop runs on copies: on the caller's arrays the compiler carries element 0 of `best` twice, one v_cndmask more
// per target (profiles/nn_scan_codeobj.txt).
template <int NORM, int Q>
__device__ __forceinline__ void scan_nearest(const float4* __restrict__ sm, int cnt, int base, const float (&qx)[Q],
                                             const float (&qy)[Q], const float (&qz)[Q], float (&best)[Q],
                                             int (&bi)[Q]) {
  float b[Q];
  int bj[Q];
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    b[k] = best[k];
    bj[k] = bi[k];
  }
#pragma unroll 4
  for (int j = 0; j < cnt; ++j) {
    const float4 p = sm[j];
#pragma unroll
    for (int k = 0; k < Q; ++k) {
      const float dd = dist3<NORM>(qx[k], qy[k], qz[k], p);
      if (dd < b[k]) {
        b[k] = dd;
        bj[k] = base + j;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    best[k] = b[k];
    bi[k] = bj[k];
  }
}

}  // namespace
