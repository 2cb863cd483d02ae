// mi355r — What the point-cloud translation units (mr_points.hip, mr_knn.hip) share: the size limits, the clamped
// cloud length, the float32 distance with its fixed operation order, and the fixed-point rows of a scatter's targets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mr_host.h"

namespace {

typedef unsigned long long u64;

inline bool sizes_ok(int64_t N, int64_t P1, int64_t P2) {
  // per-cloud indices are int32; the grid's y dimension is the batch
  return N >= 1 && P1 >= 1 && P2 >= 1 && N <= 65535 && P1 < 0x7fffffffll && P2 < 0x7fffffffll &&
         N * P1 < (1ll << 40) / 3 && N * P2 < (1ll << 40) / 3;
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

}  // namespace
