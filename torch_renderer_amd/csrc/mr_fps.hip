// mi355r — Farthest-point subsampling of point clouds (PyTorch3D sample_farthest_points): mr_farthest_points /
// mr_farthest_points_geometry / mr_farthest_points_workspace of include/mi355r.h.
//
// The rule (per cloud, L = its length, k_n = min(K[n], L)): the first index is start[n]; every point p < L carries
// m[p] = +inf; after each selection s, m[p] = min(m[p], d(p, s)) with the float32 squared distance of mr_cloud.h,
// and the next index is the p < L with the largest m[p], the lowest index among equal values. A selected point stays
// in the running with m = 0.
//
//   k_fps<T, Q, MLDS>  one workgroup of T threads (64, 256 or 1,024) owns one cloud for all of its rounds; nothing
//                 synchronises between workgroups. Thread t keeps the points q * T + t (q < Q; Q = 1, 2, 4, 8, 16, 32)
//                 in registers: x, y, z and, up to Q = 16, m. At Q = 32 (T = 1,024: four waves per SIMD, 128 registers
//                 each) the 32 m values live in LDS instead (MLDS; 128 KiB, the lane's own words, conflict free). A
//                 round: every thread updates its m values against the last winner and keeps its best as (m, q); the
//                 key (float bits of m) << 32 | ~index orders "farther, then lower index" as an unsigned integer (m >=
//                 +0); a wave takes the max of its 64 keys with four DPP steps inside each row of 16 lanes and four
//                 lane reads, reads the winner's coordinates out of the owning lane's registers, and lane 0 leaves key
//                 and coordinates in the wave's LDS slot (two sets of slots, used in turn: one __syncthreads() a round);
//                 after the barrier every wave reduces the slots the same way and reads the winning slot's coordinates.
//                 T = 64 has no LDS step and no barrier. Thread 0 stores idx[k] and pts[k]; the slots k >= k_n are
//                 written (-1 / 0) by the same launch: no memset.
//   k_fps_stream  the same loop for clouds above 1,024 * 32 points: a thread owns the strided set t, t + 1,024, ...,
//                 reads its points from global memory every round (coalesced) and keeps their m in the workspace, which
//                 nobody else touches. Correct, and slow: a round moves the whole cloud through one CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mi355r.h"
#include "mr_host.h"
#include "mr_cloud.h"

#define MRF_MAXT 1024     // threads of the largest workgroup
#define MRF_MAXQ 32       // points a thread keeps in registers, at most
#define MRF_REGQ 16       // up to this many, m is in registers too; above, in LDS
#define MRF_SLOTS 16      // waves of the largest workgroup
#define MRF_GROUP 4       // points per uniform "is any of these inside the cloud" test
#define MRF_STREAM_UNROLL 4  // points of a thread whose loads the streamed kernel keeps in flight together

namespace {

struct FpsGeom {
  int threads, q;  // q: the bucket of points per thread (streamed: the strided points per thread, unbucketed)
  bool streamed;
};

FpsGeom fps_geom(int64_t P) {
  FpsGeom g;
  g.streamed = false;
  g.threads = P <= 64 * 4 ? 64 : (P <= 256 * 8 ? 256 : MRF_MAXT);  // one wave pays no barrier
  const int64_t per = (P + g.threads - 1) / g.threads;
  if (per > MRF_MAXQ) {
    g.streamed = true;
    g.q = (int)(per < 0x7fffffff ? per : 0x7fffffff);
    return g;
  }
  g.q = 1;
  while (g.q < per) g.q *= 2;
  return g;
}

bool fps_sizes_ok(int64_t N, int64_t P, int64_t Kmax) {
  // per-cloud indices are int32; the batch is the grid's x dimension
  return N >= 1 && P >= 1 && Kmax >= 1 && N <= 0x7fffffffll && P < 0x7fffffffll && Kmax < 0x7fffffffll &&
         N * P < (1ll << 40) / 3 && N * Kmax < (1ll << 40) / 3;
}

struct FpsSlots {
  u64 key[2][MRF_SLOTS];
  float4 xyz[2][MRF_SLOTS];
};

__device__ __forceinline__ float lane_read(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

template <int CTRL> __device__ __forceinline__ u64 dpp_max(u64 v) {
  const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
  const uint32_t olo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  const uint32_t ohi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  const u64 o = ((u64)ohi << 32) | olo;
  return o > v ? o : v;
}

// The max over the 16 lanes of a DPP row, in every lane of the row: lanes ^1, ^2 (quad permutes), the mirrored half
// row (the other quad) and the mirrored row (the other half). Every lane of the wave is active at every call.
__device__ __forceinline__ u64 row_max(u64 v) {
  v = dpp_max<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_max<0x4E>(v);   // quad_perm [2,3,0,1]
  v = dpp_max<0x141>(v);  // row_half_mirror
  return dpp_max<0x140>(v);  // row_mirror
}

__device__ __forceinline__ u64 lane_read64(u64 v, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((u64)hi << 32) | lo;
}

// The max of a wave's 64 keys, wave-uniform.
__device__ __forceinline__ u64 wave_max(u64 v) {
  v = row_max(v);
  const u64 a = lane_read64(v, 0), b = lane_read64(v, 16), c = lane_read64(v, 32), d = lane_read64(v, 48);
  const u64 ab = a > b ? a : b, cd = c > d ? c : d;
  return ab > cd ? ab : cd;
}

__device__ __forceinline__ u64 fps_key(float m, uint32_t p) { return ((u64)__float_as_uint(m) << 32) | (u64)(~p); }

// A wave's best key and its point's coordinates (all wave-uniform) -> the workgroup's: cur, cx, cy, cz in every
// thread. W waves; the slots of set `buf` are free (the round before last used them, and a barrier lies between).
template <int T>
__device__ __forceinline__ void fps_pick(FpsSlots& sm, int buf, u64 wk, float wx, float wy, float wz, uint32_t& cur,
                                         float& cx, float& cy, float& cz) {
  constexpr int W = T / 64;
  if (W == 1) {
    cur = ~(uint32_t)wk;
    cx = wx, cy = wy, cz = wz;
    return;
  }
  const int lane = threadIdx.x & 63;
  if (lane == 0) {
    sm.key[buf][threadIdx.x >> 6] = wk;
    sm.xyz[buf][threadIdx.x >> 6] = make_float4(wx, wy, wz, 0.0f);
  }
  __syncthreads();
  const u64 g = row_max(sm.key[buf][lane & (W - 1)]);  // W <= 16 divides a row: every row holds every slot
  cur = ~(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)g);
  const float4 w = sm.xyz[buf][(cur & (T - 1)) >> 6];  // point p belongs to thread p % T
  cx = w.x, cy = w.y, cz = w.z;
}

// Register wq (wave-uniform, in [LO, LO + N)) of lane wl: a binary search of uniform branches down to one lane read
// per coordinate, since a register cannot be indexed at run time.
template <int LO, int N, int Q>
__device__ __forceinline__ void fps_owner_read(const float (&x)[Q], const float (&y)[Q], const float (&z)[Q], int wq,
                                               int wl, float& wx, float& wy, float& wz) {
  if constexpr (N == 1) {
    wx = lane_read(x[LO], wl);
    wy = lane_read(y[LO], wl);
    wz = lane_read(z[LO], wl);
  } else if (wq < LO + N / 2) {
    fps_owner_read<LO, N / 2, Q>(x, y, z, wq, wl, wx, wy, wz);
  } else {
    fps_owner_read<LO + N / 2, N / 2, Q>(x, y, z, wq, wl, wx, wy, wz);
  }
}

struct FpsCloud {
  const float* __restrict__ c;  // the cloud's points
  int32_t* __restrict__ oi;     // its row of idx
  float* __restrict__ op;       // its row of pts
  int64_t L, kn;                // its length; min(K[n], L)
  uint32_t start;
};

// What every kernel begins with: the cloud's rows, k_n, the clamped start index, and the padding slots written.
template <int T>
__device__ __forceinline__ FpsCloud fps_begin(const float* __restrict__ points, int64_t P,
                                              const int64_t* __restrict__ lengths, const int64_t* __restrict__ kper,
                                              int64_t Kmax, const int64_t* __restrict__ start, int32_t* __restrict__ idx,
                                              float* __restrict__ pts) {
  FpsCloud f;
  const int64_t n = blockIdx.x;
  f.L = cloud_len(lengths, n, P);
  int64_t kn = kper ? kper[n] : Kmax;
  kn = kn < 0 ? 0 : (kn > Kmax ? Kmax : kn);
  f.kn = kn < f.L ? kn : f.L;
  f.c = points + 3 * n * P;
  f.oi = idx + n * Kmax;
  f.op = pts + 3 * n * Kmax;
  for (int64_t k = f.kn + threadIdx.x; k < Kmax; k += T) {
    f.oi[k] = -1;
    f.op[3 * k] = f.op[3 * k + 1] = f.op[3 * k + 2] = 0.0f;
  }
  int64_t s = start ? start[n] : 0;
  s = s >= f.L ? f.L - 1 : s;  // a start index outside the cloud is clamped into it: nothing is read past it
  f.start = (uint32_t)(s < 0 ? 0 : s);
  return f;
}

// grid N, block T. MLDS: m in LDS (Q > MRF_REGQ).
template <int T, int Q, bool MLDS>
__global__ void __launch_bounds__(T) k_fps(const float* __restrict__ points, int64_t P,
                                           const int64_t* __restrict__ lengths, const int64_t* __restrict__ kper,
                                           int64_t Kmax, const int64_t* __restrict__ start, int32_t* __restrict__ idx,
                                           float* __restrict__ pts) {
  __shared__ FpsSlots sm;
  __shared__ float ml[MLDS ? Q * T : 1];
  constexpr int G = Q < MRF_GROUP ? Q : MRF_GROUP;
  constexpr int MQ = MLDS ? 1 : Q;
  const FpsCloud f = fps_begin<T>(points, P, lengths, kper, Kmax, start, idx, pts);
  if (f.kn == 0) return;  // uniform: the whole workgroup leaves
  const int tid = threadIdx.x;
  float x[Q], y[Q], z[Q], m[MQ];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int64_t p = (int64_t)q * T + tid;
    const bool ok = p < f.L;
    x[q] = ok ? f.c[3 * p] : 0.0f;
    y[q] = ok ? f.c[3 * p + 1] : 0.0f;
    z[q] = ok ? f.c[3 * p + 2] : 0.0f;
    // a point past the length starts at 0: a point inside the cloud has m >= +0 and a lower index, so it wins
    const float m0 = ok ? __builtin_inff() : 0.0f;
    if (MLDS) ml[q * T + tid] = m0; else m[q] = m0;
  }
  const int nq = (int)((f.L + T - 1) / T);  // groups of points at or above this q hold no point of the cloud
  uint32_t cur = f.start;
  float cx = f.c[3 * (int64_t)cur], cy = f.c[3 * (int64_t)cur + 1], cz = f.c[3 * (int64_t)cur + 2];
  for (int64_t k = 0;; ++k) {
    if (tid == 0) {
      f.oi[k] = (int32_t)cur;
      f.op[3 * k] = cx;
      f.op[3 * k + 1] = cy;
      f.op[3 * k + 2] = cz;
    }
    if (k + 1 >= f.kn) break;
    const float4 w = make_float4(cx, cy, cz, 0.0f);
    float bm = -1.0f;  // every m is >= +0
    int bq = 0;
#pragma unroll
    for (int q0 = 0; q0 < Q; q0 += G) {
      if (q0 < nq) {  // uniform
#pragma unroll
        for (int q = q0; q < q0 + G; ++q) {
          const float d = dist3<2>(x[q], y[q], z[q], w);
          float mq;
          if (MLDS) {
            mq = fminf(ml[q * T + tid], d);
            ml[q * T + tid] = mq;
          } else {
            mq = m[q] = fminf(m[q], d);
          }
          if (mq > bm) bm = mq, bq = q;  // ascending q: an equal value keeps the lower index
        }
      }
    }
    const u64 wk = wave_max(fps_key(bm, (uint32_t)(bq * T + tid)));
    const uint32_t wp = ~(uint32_t)wk;  // the wave's winner: thread wp % T, register wp / T
    const int wl = (int)(wp & 63u), wq = (int)(wp / (uint32_t)T);
    float wx, wy, wz;
    fps_owner_read<0, Q>(x, y, z, wq, wl, wx, wy, wz);
    fps_pick<T>(sm, (int)(k & 1), wk, wx, wy, wz, cur, cx, cy, cz);
  }
}

// grid N, block MRF_MAXT. m: (N, P) floats of the workspace.
__global__ void __launch_bounds__(MRF_MAXT) k_fps_stream(const float* __restrict__ points, int64_t P,
                                                         const int64_t* __restrict__ lengths,
                                                         const int64_t* __restrict__ kper, int64_t Kmax,
                                                         const int64_t* __restrict__ start, int32_t* __restrict__ idx,
                                                         float* __restrict__ pts, float* __restrict__ mws) {
  __shared__ FpsSlots sm;
  constexpr int T = MRF_MAXT;
  const FpsCloud f = fps_begin<T>(points, P, lengths, kper, Kmax, start, idx, pts);
  if (f.kn == 0) return;
  const int tid = threadIdx.x;
  float* __restrict__ m = mws + (int64_t)blockIdx.x * P;
  for (int64_t p = tid; p < f.L; p += T) m[p] = __builtin_inff();  // read back by this thread alone
  uint32_t cur = f.start;
  float cx = f.c[3 * (int64_t)cur], cy = f.c[3 * (int64_t)cur + 1], cz = f.c[3 * (int64_t)cur + 2];
  for (int64_t k = 0;; ++k) {
    if (tid == 0) {
      f.oi[k] = (int32_t)cur;
      f.op[3 * k] = cx;
      f.op[3 * k + 1] = cy;
      f.op[3 * k + 2] = cz;
    }
    if (k + 1 >= f.kn) break;
    const float4 w = make_float4(cx, cy, cz, 0.0f);
    float bm = -1.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
    uint32_t bp = 0;
    auto visit = [&](int64_t p, float px, float py, float pz, float mo) {
      const float mp = fminf(mo, dist3<2>(px, py, pz, w));
      m[p] = mp;
      if (mp > bm) bm = mp, bp = (uint32_t)p, bx = px, by = py, bz = pz;  // ascending p: ties keep the lower index
    };
    int64_t p = tid;
    for (; p + (MRF_STREAM_UNROLL - 1) * T < f.L; p += MRF_STREAM_UNROLL * T) {  // the loads of four points in flight
      float px[MRF_STREAM_UNROLL], py[MRF_STREAM_UNROLL], pz[MRF_STREAM_UNROLL], mo[MRF_STREAM_UNROLL];
#pragma unroll
      for (int j = 0; j < MRF_STREAM_UNROLL; ++j) {
        const int64_t q = p + j * T;
        px[j] = f.c[3 * q], py[j] = f.c[3 * q + 1], pz[j] = f.c[3 * q + 2], mo[j] = m[q];
      }
#pragma unroll
      for (int j = 0; j < MRF_STREAM_UNROLL; ++j) visit(p + j * T, px[j], py[j], pz[j], mo[j]);
    }
    for (; p < f.L; p += T) visit(p, f.c[3 * p], f.c[3 * p + 1], f.c[3 * p + 2], m[p]);
    // a thread without a point of the cloud offers the key 0, below every key of a point (~p >= 2^31)
    const u64 wk = wave_max(tid < f.L ? fps_key(bm, bp) : 0ull);
    const int wl = (int)(~(uint32_t)wk & 63u);  // p % 1,024 % 64: the owning lane
    fps_pick<T>(sm, (int)(k & 1), wk, lane_read(bx, wl), lane_read(by, wl), lane_read(bz, wl), cur, cx, cy, cz);
  }
}

}  // namespace

extern "C" {

int32_t mr_farthest_points_geometry(int64_t N, int64_t P, int64_t Kmax, int32_t* threads, int32_t* points_per_thread,
                                    int32_t* streamed) {
  if (N < 1 || P < 1 || Kmax < 1) return set_err(MR_EINVAL, "farthest points geometry: N, P and Kmax must be >= 1");
  if (!fps_sizes_ok(N, P, Kmax))
    return set_err(MR_EUNSUPPORTED, "farthest points geometry: clouds too large for 32-bit point ids");
  const FpsGeom g = fps_geom(P);
  if (threads) *threads = g.threads;
  if (points_per_thread) *points_per_thread = g.q;
  if (streamed) *streamed = g.streamed ? 1 : 0;
  return MR_OK;
}

size_t mr_farthest_points_workspace(int64_t N, int64_t P, int64_t Kmax) {
  if (!fps_sizes_ok(N, P, Kmax)) return 0;
  Carver c(nullptr);
  c.take<float>((fps_geom(P).streamed ? (size_t)(N * P) : 0) + 1);  // never 0: 0 means out of range
  return c.off;
}

int32_t mr_farthest_points(const float* points, int64_t N, int64_t P, const int64_t* lengths, const int64_t* K_per_cloud,
                           int64_t Kmax, const int64_t* start_idx, int32_t* idx, float* pts, void* ws, size_t ws_bytes,
                           void* stream) {
  if (N < 1 || P < 1 || Kmax < 1) return set_err(MR_EINVAL, "farthest points: N, P and Kmax must be >= 1");
  if (!fps_sizes_ok(N, P, Kmax))
    return set_err(MR_EUNSUPPORTED, "farthest points: clouds too large for 32-bit point ids");
  if (!points || !idx || !pts || !ws) return set_err(MR_EINVAL, "farthest points: points / idx / pts / workspace is NULL");
  if (ws_bytes < mr_farthest_points_workspace(N, P, Kmax))
    return set_err(MR_EWORKSPACE, "farthest points workspace too small");
  const FpsGeom g = fps_geom(P);
  const hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)N;
  if (g.streamed)
    return launch(KID_NONE, "k_fps_stream", k_fps_stream, grid, MRF_MAXT, 0, st, points, P, lengths, K_per_cloud, Kmax,
                  start_idx, idx, pts, (float*)ws);
#define MRF_CASE(T, Q)                                                                                              \
  case T + Q:                                                                                                       \
    return launch(KID_NONE, "k_fps", k_fps<T, Q, (Q > MRF_REGQ)>, grid, T, 0, st, points, P, lengths, K_per_cloud, \
                  Kmax, start_idx, idx, pts)
  switch (g.threads + g.q) {  // the thread counts are multiples of 64 and q <= 32: the sums are distinct
    MRF_CASE(64, 1);
    MRF_CASE(64, 2);
    MRF_CASE(64, 4);
    MRF_CASE(256, 2);
    MRF_CASE(256, 4);
    MRF_CASE(256, 8);
    MRF_CASE(1024, 4);
    MRF_CASE(1024, 8);
    MRF_CASE(1024, 16);
    MRF_CASE(1024, 32);
  }
#undef MRF_CASE
  return set_err(MR_EINVAL, "farthest points: no kernel for %d threads x %d points", g.threads, g.q);
}

}  // extern "C"
