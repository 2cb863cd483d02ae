// mi355r — What the ICP estimators of mr_points.hip (iterative_closest_point, ..._to_plane) and of mr_icpmesh.hip
// (..._to_mesh) share: the loop's workspace (mr_icp_init's layout), the status words, and the float64 Gauss-Newton
// step of the point-to-plane residual: a pair's terms of the normal equations, the damped 6x6 solve with its update,
// the solve kernel with the new residual, and the status kernel. The rule is stated in include/mi355r.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mr_common.h"
#include "mr_host.h"
#include "mr_cloud.h"

#define MRR_BLOCK 256                  // threads of the kernels that are not scans
#define MRR_PER 4                      // points per thread of a tile
#define MRR_TILE (MRR_BLOCK * MRR_PER)

#define MRI_RTS 13
#define MRI_XC 8        // per-cloud constants (double): sum w, mean of x (3), sum w |x - mean|^2, sum w (x - mean) (3)
#define MRI_MOM 12      // per-workgroup moments (double): sum w y (3), sum w (x - mean) y^T (9, row = x component)
#define MRI_PMOM 28     // per-workgroup sums (double): A's upper triangle row by row (21), b (6), the pair count m

namespace {

struct IcpWS {
  u64* key;       // (N, P1), all-ones between iterations (the moments kernel resets what it reads)
  int32_t* idx;   // (N, P1) this iteration's neighbours, -1 for no term
  double* xc;     // (N, MRI_XC)
  double* mom;    // (N, nblk, MRI_MOM)
  double* res;    // (N, nblk)
  int64_t nblk;
  size_t key_bytes, bytes;
};
inline IcpWS carve_icp(void* base, int64_t N, int64_t P1) {
  IcpWS w;
  Carver c(base);
  w.key_bytes = sizeof(u64) * (size_t)(N * P1);
  w.key = c.take<u64>((size_t)(N * P1));
  w.idx = c.take<int32_t>((size_t)(N * P1));
  w.xc = c.take<double>((size_t)(N * MRI_XC));
  w.nblk = ceil_div(P1, MRR_TILE);
  w.mom = c.take<double>((size_t)(N * w.nblk * MRI_MOM));
  w.res = c.take<double>((size_t)(N * w.nblk));
  w.bytes = c.off;
  return w;
}

struct IcpPlaneWS {
  IcpWS icp;      // mr_icp_init's layout comes first: the init is shared
  double* pmom;   // (N, nblk, MRI_PMOM)
  double* cnt;    // (N) valid pairs of this iteration
  float* prev;    // (N, MRI_RTS) the transform the iteration started from (rts is overwritten while tiles still solve)
  size_t bytes;
};
inline IcpPlaneWS carve_icp_plane(void* base, int64_t N, int64_t P1) {
  IcpPlaneWS w;
  w.icp = carve_icp(base, N, P1);
  Carver c(base, w.icp.bytes);
  w.pmom = c.take<double>((size_t)(N * w.icp.nblk * MRI_PMOM));
  w.cnt = c.take<double>((size_t)N);
  w.prev = c.take<float>((size_t)(N * MRI_RTS));
  w.bytes = c.off;
  return w;
}

// K sums over a workgroup of WAVES waves: the butterfly inside each wave, then wave 0 + wave 1 (+ wave 2 + wave 3,
// block_sum's tree). sm: WAVES * K doubles. Every thread gets the totals.
template <int WAVES, int K> __device__ __forceinline__ void block_sums(double (&v)[K], double* sm) {
#pragma unroll
  for (int k = 0; k < K; ++k)
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) sm[(threadIdx.x >> 6) * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    v[k] = sm[k];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v[k] += sm[w * K + k];
  }
  __syncthreads();
}

// status[0]: the batch has converged; status[1]: iterations run. An iteration's kernels do nothing once either
// the batch has converged or max_iter iterations have run (the host may enqueue more than are needed).
__device__ __forceinline__ bool icp_idle(const int32_t* __restrict__ status, int max_iter) {
  return status && (status[0] != 0 || status[1] >= max_iter || status[1] < 0);
}

// c = s (mx R) + T in float64 from the float32 transform t and the cloud's constants (xc[1..3] = mx).
__host__ __device__ __forceinline__ void plane_centre(const double* __restrict__ xc, const float* __restrict__ t,
                                                      double (&c)[3]) {
  const double s = (double)t[12];
  for (int b = 0; b < 3; ++b)
    c[b] = s * ((xc[1] * (double)t[b] + xc[2] * (double)t[3 + b]) + xc[3] * (double)t[6 + b]) + (double)t[9 + b];
}

// Step 2 of the rule for one valid pair, in float64: p the transformed source point, q its counterpart with the
// normal nn, c the centre: r = (p - q).n, J = [(p - c) x n, n]; a += (J J^T's upper triangle, J r, 1).
__device__ __forceinline__ void plane_accum(float p0, float p1, float p2, const float* __restrict__ t,
                                            const float* __restrict__ nn, const double (&c)[3],
                                            double (&a)[MRI_PMOM]) {
  const double n0 = (double)nn[0], n1 = (double)nn[1], n2 = (double)nn[2];
  const double d0 = (double)p0 - (double)t[0], d1 = (double)p1 - (double)t[1], d2 = (double)p2 - (double)t[2];
  const double u0 = (double)p0 - c[0], u1 = (double)p1 - c[1], u2 = (double)p2 - c[2];
  const double r = (d0 * n0 + d1 * n1) + d2 * n2;
  const double J[6] = {u1 * n2 - u2 * n1, u2 * n0 - u0 * n2, u0 * n1 - u1 * n0, n0, n1, n2};
  int e = 0;
#pragma unroll
  for (int v = 0; v < 6; ++v)
#pragma unroll
    for (int w = v; w < 6; ++w) a[e++] += J[v] * J[w];
#pragma unroll
  for (int v = 0; v < 6; ++v) a[21 + v] += J[v] * r;
  a[27] += 1.0;
}

// The workgroup's sums of plane_accum -> pmom[(n, block)]. sm: 4 * MRI_PMOM doubles.
__device__ __forceinline__ void plane_store(double (&a)[MRI_PMOM], double* sm, double* __restrict__ pmom, int64_t n,
                                            int64_t nblk) {
  block_sums<MRR_BLOCK / 64>(a, sm);
  if (threadIdx.x < MRI_PMOM) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < MRI_PMOM; ++k) v = threadIdx.x == k ? a[k] : v;
    pmom[(n * nblk + blockIdx.x) * MRI_PMOM + threadIdx.x] = v;
  }
}

// Steps 3 and 4 of the rule, in float64: xi = (w, t) solves (A + lam I) xi = -b, lam = 1e-9 trace(A) / 6, by a 6x6
// Cholesky; E = exp([w]x) by Rodrigues (the series 1 - th^2/6, 1/2 - th^2/24 below th = 1e-4); R <- R E^T,
// T <- (T - c) E^T + c + t, s as it is, rounded once to float32. A: the 21 entries of the upper triangle row by row.
// trace(A) not > 0 (no pair, only zero normals, a NaN), a pivot not > 0 or a non-finite solution: xi = 0 and `out`
// is `in`, bit for bit.
// (Also a host function: mr_icp_plane_solve_host.)
__host__ __device__ inline void plane_step(const double* __restrict__ A, const double* __restrict__ b,
                                           const float* __restrict__ in, const double (&c)[3], float* out) {
  double L[6][6], xi[6];
  double tr = 0.0;
  {
    int e = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) {
        L[i][j] = L[j][i] = A[e++];
        if (i == j) tr += L[i][i];
      }
  }
  bool ok = tr > 0.0;
  if (ok) {
    const double lam = 1e-9 * tr / 6.0;
    for (int j = 0; j < 6 && ok; ++j) {  // the lower triangle becomes the Cholesky factor
      double d = L[j][j] + lam;
      for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
      ok = d > 0.0;
      if (!ok) break;
      d = sqrt(d);
      L[j][j] = d;
      for (int i = j + 1; i < 6; ++i) {
        double v = L[i][j];
        for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
        L[i][j] = v / d;
      }
    }
  }
  if (ok) {
    for (int i = 0; i < 6; ++i) {  // L z = -b
      double v = -b[i];
      for (int k = 0; k < i; ++k) v -= L[i][k] * xi[k];
      xi[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {  // L^T xi = z
      double v = xi[i];
      for (int k = i + 1; k < 6; ++k) v -= L[k][i] * xi[k];
      xi[i] = v / L[i][i];
    }
    for (int i = 0; i < 6; ++i) ok = ok && (xi[i] - xi[i] == 0.0);  // finite
  }
  if (!ok) {
    for (int k = 0; k < MRI_RTS; ++k) out[k] = in[k];
    return;
  }
  const double w0 = xi[0], w1 = xi[1], w2 = xi[2];
  const double th2 = (w0 * w0 + w1 * w1) + w2 * w2, th = sqrt(th2);
  double ka, kb;
  if (th < 1e-4) {
    ka = 1.0 - th2 / 6.0;
    kb = 0.5 - th2 / 24.0;
  } else {
    ka = sin(th) / th;
    kb = (1.0 - cos(th)) / th2;
  }
  const double dg = 1.0 - kb * th2;
  const double E[3][3] = {{dg + kb * w0 * w0, kb * w0 * w1 - ka * w2, kb * w0 * w2 + ka * w1},
                          {kb * w1 * w0 + ka * w2, dg + kb * w1 * w1, kb * w1 * w2 - ka * w0},
                          {kb * w2 * w0 - ka * w1, kb * w2 * w1 + ka * w0, dg + kb * w2 * w2}};
  for (int a = 0; a < 3; ++a)
    for (int k = 0; k < 3; ++k)
      out[3 * a + k] = (float)(((double)in[3 * a] * E[k][0] + (double)in[3 * a + 1] * E[k][1]) +
                               (double)in[3 * a + 2] * E[k][2]);
  const double u0 = (double)in[9] - c[0], u1 = (double)in[10] - c[1], u2 = (double)in[11] - c[2];
  for (int k = 0; k < 3; ++k) out[9 + k] = (float)((((u0 * E[k][0] + u1 * E[k][1]) + u2 * E[k][2]) + c[k]) + xi[3 + k]);
  out[12] = in[12];
}

// grid (nblk, N). Thread 0 of every workgroup sums its cloud's partials in order and takes the step from prev (the
// same inputs and code: the same bits in every workgroup of the cloud); workgroup 0 stores the transform in rts and
// in slot status[1] of the history, and the pair count in cnt. Then the workgroup's tile of the new residual
// sum ((p' - q).n)^2 over this iteration's valid pairs, p' = sim_apply of the new transform; source point i pairs
// with row idx[i] of y and yn (N, P2, 3), idx[i] < 0: no pair.
__global__ void __launch_bounds__(MRR_BLOCK) k_icp_plane_solve(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ yn, int64_t N, int64_t P1,
    int64_t P2, const int64_t* __restrict__ xl, const double* __restrict__ xc, const double* __restrict__ pmom,
    int64_t nblk, const int32_t* __restrict__ idx, const float* __restrict__ prev, const int32_t* __restrict__ status,
    int max_iter, float* __restrict__ rts, float* __restrict__ hist, double* __restrict__ cnt,
    double* __restrict__ res) {
  __shared__ double sm[4];
  __shared__ float tr[MRI_RTS];
  if (icp_idle(status, max_iter)) return;
  const int64_t n = blockIdx.y;
  if (threadIdx.x == 0) {
    double m[MRI_PMOM];
    for (int k = 0; k < MRI_PMOM; ++k) m[k] = 0.0;
    for (int64_t b = 0; b < nblk; ++b)
      for (int k = 0; k < MRI_PMOM; ++k) m[k] += pmom[(n * nblk + b) * MRI_PMOM + k];
    double c[3];
    plane_centre(xc + n * MRI_XC, prev + n * MRI_RTS, c);
    plane_step(m, m + 21, prev + n * MRI_RTS, c, tr);
    if (blockIdx.x == 0) cnt[n] = m[27];
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x < MRI_RTS) {
    rts[n * MRI_RTS + threadIdx.x] = tr[threadIdx.x];
    hist[((int64_t)status[1] * N + n) * MRI_RTS + threadIdx.x] = tr[threadIdx.x];
  }
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
    const float* __restrict__ nn = yn + 3 * (n * P2 + j);
    float o0, o1, o2;
    sim_apply(tr, q[0], q[1], q[2], o0, o1, o2);
    const double d0 = (double)o0 - (double)t[0], d1 = (double)o1 - (double)t[1], d2 = (double)o2 - (double)t[2];
    const double r = (d0 * (double)nn[0] + d1 * (double)nn[1]) + d2 * (double)nn[2];
    acc += r * r;
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) res[n * nblk + blockIdx.x] = acc;
}

// k_icp_status with the pair count as divisor: rmse = sqrt(residual / max(m, 1)); a cloud without a valid pair
// (rmse 0) counts as done. rmse holds the previous iteration's values on entry.
__global__ void __launch_bounds__(MRR_BLOCK) k_icp_plane_status(const double* __restrict__ res, int64_t nblk, int64_t N,
                                                                const double* __restrict__ cnt, float thr,
                                                                int max_iter, float* __restrict__ rmse,
                                                                int32_t* __restrict__ status) {
  __shared__ double sm[4];
  if (icp_idle(status, max_iter)) return;  // uniform
  const int it = status[1];
  double open = 0.0;
  for (int64_t n = threadIdx.x; n < N; n += MRR_BLOCK) {
    double s = 0.0;
    for (int64_t b = 0; b < nblk; ++b) s += res[n * nblk + b];
    const double m = cnt[n];
    const float r = (float)sqrt(s / (m > 1.0 ? m : 1.0));
    const float prev = rmse[n];
    const float rel = it == 0 ? 1.0f : (prev - r) / prev;
    if (!(rel <= thr) && m != 0.0) open += 1.0;
    rmse[n] = r;
  }
  open = block_sum(open, sm);  // also orders every thread's read of status[1] before its update
  if (threadIdx.x == 0) {
    status[1] = it + 1;
    if (open == 0.0) status[0] = 1;
  }
}

}  // namespace
