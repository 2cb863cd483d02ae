// mi355r — point-cloud rendering (PyTorch3D rasterize_points with naive semantics, alpha_composite and
// norm_weighted_sum, the points' world -> NDC projection): mr_project_points* / mr_rasterize_points* /
// mr_composite_points* of include/mi355r.h. A translation unit of its own: no kernel of the mesh path is touched.
//
//   k_point_raster      a workgroup owns one (view, macro-tile) at a time (grid-stride): four waves a 16x16 tile, or
//                       one wave an 8x8 tile when the K-deep lists of four would not fit 64 KiB of LDS. One pixel per
//                       lane. The view's cloud streams through in chunks of MRP_CHUNK points: every thread loads
//                       points, drops those whose disc cannot reach a pixel centre of the macro-tile (a float32
//                       bound that is never larger than any pixel's own d2, see tile_d2) and the wave compacts the
//                       survivors into LDS with a ballot; then every lane runs the exact test d2 < r2 on the
//                       survivors and inserts (z bits << 32 | point) into its ascending K-deep list (lane-strided
//                       LDS, as mr_kdeep.h's). z >= 0, so the float bits order as integers (-0.0 is stored as +0.0);
//                       the key order is total, so the result does not depend on the scan order. No capacity, no
//                       overflow path, no global lists: the cost is N * tiles * P coarse tests.
//   k_point_raster_bwd  one thread per (pixel, slot): adds (g_dists 2 dx, g_dists 2 dy, g_zbuf) to the point's row
//                       with the 64-bit fixed-point atomics of mr_common.h; k_pr_fix_to_float writes the floats.
//   k_project_points    world -> view -> NDC of every (view, point), the operand order of the mesh projection.
//   k_project_points_bwd one workgroup per view: the points' gradients through the fixed-point rows (summed over the
//                       views that share a cloud), the view's R / T gradient from float64 sums in a fixed tree.
//   k_composite_fwd/bwd one pixel per thread, any C (four channels at a time), alpha or norm-weighted by a flag,
//                       alpha = 1 - dists / r^2 formed in the kernel when asked, the background applied in the kernel;
//                       feature gradients through the fixed-point rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mi355r.h"
#include "mr_common.h"
#include "mr_host.h"

#define MRP_CHUNK 256   // points staged per pass (mr_point_raster_chunk)
#define MRP_SEG 64      // one wave's share of a chunk
#define MRP_KMAX 50     // deepest per-pixel list
#define MRP_K4 28       // deepest list for which four waves' lists fit 64 KiB of LDS
#define MRP_BLOCK 256

namespace {

typedef unsigned long long u64;

struct FixRows {
  u64* fix;
  float* rem;
  size_t bytes;
};
FixRows carve_rows(void* base, int64_t n) {
  FixRows w;
  Carver c(base);
  w.fix = c.take_packed<u64>((size_t)n);  // words and remainders back to back: one memset
  w.rem = c.take<float>((size_t)n);
  w.bytes = c.off;
  return w;
}

__global__ void __launch_bounds__(MRP_BLOCK) k_pr_fix_to_float(const u64* __restrict__ fix, const float* __restrict__ rem,
                                                               int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * MRP_BLOCK + threadIdx.x;
  if (i < n) out[i] = fix_read(fix, rem, i);
}

// ------------------------------------------------------------------------------------------- rasterization
struct PointRasterParams {
  const float* pts;         // (total, 3) NDC x, NDC y, view z
  const int64_t* first;     // (N) first row of view n's cloud
  const int64_t* count;     // (N)
  const int64_t* idx_base;  // (N) or NULL: idx = idx_base[n] + (row - first[n]); NULL: the row itself
  const float* radius;      // (total) or NULL
  float r0;
  int64_t N, total;
  int H, W, K, mtx, mty;
  int64_t* idx;
  float* zbuf;
  float* dists;
};

// A lower bound, in float32, of every d2 = dx*dx + dy*dy (dx = px - xf, dy = py - yf) over the pixel centres
// xf in [xlo, xhi], yf in [ylo, yhi]: the same expression at the nearest edge. Float subtraction, multiplication and
// addition are monotonic, so the bound holds after rounding too: a point with !(bound < r2) covers no pixel.
MR_DEV float tile_d2(float px, float py, float xlo, float xhi, float ylo, float yhi) {
  const float dx = px > xhi ? px - xhi : (px < xlo ? px - xlo : 0.0f);
  const float dy = py > yhi ? py - yhi : (py < ylo ? py - ylo : 0.0f);
  return dx * dx + dy * dy;
}

template <int NW>
__global__ void __launch_bounds__(64 * NW) k_point_raster(PointRasterParams P) {
  constexpr int NT = 64 * NW;
  constexpr int MT = NW == 4 ? 16 : 8;  // macro-tile side
  constexpr int SPW = MRP_CHUNK / MRP_SEG / NW;  // segments of a chunk per wave
  extern __shared__ __align__(16) unsigned char smem[];
  u64* const lists = (u64*)smem;                            // [K][NT], lane-strided
  float4* const sv = (float4*)(lists + (size_t)P.K * NT);   // [MRP_CHUNK] survivors: x, y, z bits, r2
  int* const si = (int*)(sv + MRP_CHUNK);                   // [MRP_CHUNK] their point (within the cloud)
  __shared__ int scnt[MRP_CHUNK / MRP_SEG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  u64* const mine = lists + tid;
  const int K = P.K;
  const int64_t tiles = (int64_t)P.mtx * P.mty, total = P.N * tiles;
  for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
    const int64_t n = t / tiles;
    const int tt = (int)(t - n * tiles);
    const int X0 = (tt % P.mtx) * MT, Y0 = (tt / P.mtx) * MT;
    const int px = X0 + (NW == 4 ? (wave & 1) * 8 : 0) + (lane & 7);
    const int py = Y0 + (NW == 4 ? (wave >> 1) * 8 : 0) + (lane >> 3);
    const bool in_img = px < P.W && py < P.H;
    const float xf = col_ndc(in_img ? px : 0, P.H, P.W), yf = row_ndc(in_img ? py : 0, P.H, P.W);
    // NDC runs against the pixel index (both axes are flipped)
    const float xhi = col_ndc(X0, P.H, P.W), xlo = col_ndc(min(X0 + MT, P.W) - 1, P.H, P.W);
    const float yhi = row_ndc(Y0, P.H, P.W), ylo = row_ndc(min(Y0 + MT, P.H) - 1, P.H, P.W);
    const int64_t first = P.first[n];
    int64_t cnt = P.count[n];
    if (first < 0 || cnt < 0 || first + cnt > P.total) cnt = 0;
    const float* __restrict__ pts = P.pts + 3 * first;
    const float* __restrict__ rad = P.radius ? P.radius + first : nullptr;
    int filled = 0;
    u64 worst = ~0ull;  // the list's last key once it is full
    // this thread's points of the next chunk, loaded one chunk ahead: the loads' latency passes under the scan
    float nx[SPW], ny[SPW], nz[SPW], nr[SPW];
    auto fetch = [&](int64_t c0) {
#pragma unroll
      for (int u = 0; u < SPW; ++u) {
        const int64_t i = c0 + (wave + u * NW) * MRP_SEG + lane;
        const bool ok = i < cnt;
        nx[u] = ok ? pts[3 * i] : 0.0f;
        ny[u] = ok ? pts[3 * i + 1] : 0.0f;
        nz[u] = ok ? pts[3 * i + 2] : -1.0f;
        nr[u] = ok && rad ? rad[i] : P.r0;
      }
    };
    fetch(0);
    for (int64_t c0 = 0; c0 < cnt; c0 += MRP_CHUNK) {
      float cx[SPW], cy[SPW], cz[SPW], cr[SPW];
#pragma unroll
      for (int u = 0; u < SPW; ++u) {
        cx[u] = nx[u];
        cy[u] = ny[u];
        cz[u] = nz[u];
        cr[u] = nr[u];
      }
      if (c0 + MRP_CHUNK < cnt) fetch(c0 + MRP_CHUNK);
#pragma unroll
      for (int u = 0; u < SPW; ++u) {
        const int s = wave + u * NW;
        const int64_t i = c0 + s * MRP_SEG + lane;
        const float x = cx[u], y = cy[u], z = cz[u], r2 = cr[u] * cr[u];
        // a slot past the cloud holds z = -1; NaN z: not drawn
        const bool keep = z >= 0.0f && tile_d2(x, y, xlo, xhi, ylo, yhi) < r2;
        const u64 m = __ballot(keep);
        if (keep) {
          const int pos = s * MRP_SEG + __popcll(m & ((1ull << lane) - 1ull));
          sv[pos] = make_float4(x, y, z == 0.0f ? 0.0f : z, r2);  // -0.0 -> +0.0
          si[pos] = (int)i;
        }
        if (lane == 0) scnt[s] = __popcll(m);
      }
      __syncthreads();
      if (in_img) {
        for (int s = 0; s < MRP_CHUNK / MRP_SEG; ++s) {
          const int ns = scnt[s];
          for (int j = 0; j < ns; ++j) {
            const float4 q = sv[s * MRP_SEG + j];
            const float dx = q.x - xf, dy = q.y - yf;
            const float d2 = dx * dx + dy * dy;
            if (!(d2 < q.w)) continue;
            const u64 key = ((u64)__float_as_uint(q.z) << 32) | (u64)(uint32_t)si[s * MRP_SEG + j];
            if (!(key < worst)) continue;
            int k = filled < K ? filled : K - 1;
            while (k > 0) {
              const u64 prev = mine[(size_t)(k - 1) * NT];
              if (prev < key) break;
              mine[(size_t)k * NT] = prev;
              --k;
            }
            mine[(size_t)k * NT] = key;
            if (filled < K) ++filled;
            if (filled == K) worst = mine[(size_t)(K - 1) * NT];
          }
        }
      }
      __syncthreads();
    }
    if (in_img) {
      const int64_t o = ((n * P.H + py) * (int64_t)P.W + px) * K;
      const int64_t ib = P.idx_base ? P.idx_base[n] : first;
      for (int k = 0; k < K; ++k) {
        if (k < filled) {
          const u64 key = mine[(size_t)k * NT];
          const int64_t p = (int64_t)(uint32_t)key;
          const float dx = pts[3 * p] - xf, dy = pts[3 * p + 1] - yf;
          P.idx[o + k] = ib + p;
          P.zbuf[o + k] = __uint_as_float((uint32_t)(key >> 32));
          P.dists[o + k] = dx * dx + dy * dy;
        } else {
          P.idx[o + k] = -1;
          P.zbuf[o + k] = -1.0f;
          P.dists[o + k] = -1.0f;
        }
      }
    }
  }
}

__global__ void __launch_bounds__(MRP_BLOCK) k_point_raster_bwd(const float* __restrict__ pts,
                                                                const int64_t* __restrict__ first,
                                                                const int64_t* __restrict__ idx_base, int64_t total,
                                                                int64_t nslots, int H, int W, int K,
                                                                const int64_t* __restrict__ idx,
                                                                const float* __restrict__ gz,
                                                                const float* __restrict__ gd, u64* __restrict__ fix,
                                                                float* __restrict__ rem) {
  const int64_t t = (int64_t)blockIdx.x * MRP_BLOCK + threadIdx.x;
  if (t >= nslots) return;
  const int64_t i = idx[t];
  if (i < 0) return;
  const int64_t pix = t / K;
  const int xi = (int)(pix % W), yi = (int)((pix / W) % H);
  const int64_t n = pix / ((int64_t)W * H);
  const int64_t src = idx_base ? first[n] + (i - idx_base[n]) : i;
  if (src < 0 || src >= total) return;
  if (gd) {
    const float g2 = gd[t] * 2.0f;
    fix_add(fix, rem, 3 * src, g2 * (pts[3 * src] - col_ndc(xi, H, W)));
    fix_add(fix, rem, 3 * src + 1, g2 * (pts[3 * src + 1] - row_ndc(yi, H, W)));
  }
  if (gz) fix_add(fix, rem, 3 * src + 2, gz[t]);
}

// ------------------------------------------------------------------------------------------- projection
// views (N,16): R (9, row vectors: view = X R + T), T (3), ax, bx, ay, by.
__global__ void __launch_bounds__(MRP_BLOCK) k_project_points(const float* __restrict__ pts,
                                                              const int64_t* __restrict__ src_first,
                                                              const int64_t* __restrict__ dst_first,
                                                              const int64_t* __restrict__ count,
                                                              const float* __restrict__ views,
                                                              float* __restrict__ out) {
  const int64_t n = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * MRP_BLOCK + threadIdx.x;
  if (i >= count[n]) return;
  const float* __restrict__ v = views + 16 * n;
  const float* __restrict__ X = pts + 3 * (src_first[n] + i);
  const float vx = ((X[0] * v[0] + X[1] * v[3]) + X[2] * v[6]) + v[9];
  const float vy = ((X[0] * v[1] + X[1] * v[4]) + X[2] * v[7]) + v[10];
  const float vz = ((X[0] * v[2] + X[1] * v[5]) + X[2] * v[8]) + v[11];
  float* __restrict__ o = out + 3 * (dst_first[n] + i);
  o[0] = v[12] * (vx / vz) + v[13];
  o[1] = v[14] * (vy / vz) + v[15];
  o[2] = vz;
}

// grid (N): gviews (N,12) = d / d (R, T) of view n, the points' gradients into the fixed-point rows.
__global__ void __launch_bounds__(MRP_BLOCK) k_project_points_bwd(const float* __restrict__ pts,
                                                                  const int64_t* __restrict__ src_first,
                                                                  const int64_t* __restrict__ dst_first,
                                                                  const int64_t* __restrict__ count,
                                                                  const float* __restrict__ views,
                                                                  const float* __restrict__ g, u64* __restrict__ fix,
                                                                  float* __restrict__ rem,
                                                                  float* __restrict__ gviews) {
  __shared__ double sm[4];
  const int64_t n = blockIdx.x;
  const float* __restrict__ v = views + 16 * n;
  const int64_t cnt = count[n], s0 = src_first[n], d0 = dst_first[n];
  double acc[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) acc[q] = 0.0;
  for (int64_t i = threadIdx.x; i < cnt; i += MRP_BLOCK) {
    const float* __restrict__ X = pts + 3 * (s0 + i);
    const float* __restrict__ gi = g + 3 * (d0 + i);
    const float vx = ((X[0] * v[0] + X[1] * v[3]) + X[2] * v[6]) + v[9];
    const float vy = ((X[0] * v[1] + X[1] * v[4]) + X[2] * v[7]) + v[10];
    const float vz = ((X[0] * v[2] + X[1] * v[5]) + X[2] * v[8]) + v[11];
    const float iz = 1.0f / vz;
    float gv[3];
    gv[0] = gi[0] * v[12] * iz;
    gv[1] = gi[1] * v[14] * iz;
    gv[2] = gi[2] - (gv[0] * vx + gv[1] * vy) * iz;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      fix_add(fix, rem, 3 * (s0 + i) + r, (v[3 * r] * gv[0] + v[3 * r + 1] * gv[1]) + v[3 * r + 2] * gv[2]);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[3 * r + c] += (double)X[r] * (double)gv[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[9 + c] += (double)gv[c];
  }
#pragma unroll
  for (int q = 0; q < 12; ++q) {
    const double tot = block_sum(acc[q], sm);
    if (threadIdx.x == 0) gviews[12 * n + q] = (float)tot;
  }
}

// ------------------------------------------------------------------------------------------- compositing
struct CompositeParams {
  const int64_t* idx;     // (npix, K)
  const float* vals;      // (npix, K) alphas, or dists with MR_COMPOSITE_DISTS
  const float* feats;     // (P, C)
  const float* radius;    // (nrad) indexed by idx, or NULL
  const int64_t* feat_sub;  // (N) or NULL: feature row = idx - feat_sub[n]
  const float* bg;        // (C) or NULL
  int64_t npix, hw, P, nrad;
  int K, C, flags;
  float r0;
};

struct Slot {
  int64_t row;
  float a, r2;
};
// Slot k of pixel `pix`: false for an empty slot (or an index outside the features / radii: never read).
MR_DEV bool comp_slot(const CompositeParams& P, int64_t pix, int64_t sub, int k, Slot& s) {
  const int64_t i = P.idx[pix * P.K + k];
  if (i < 0) return false;
  s.row = i - sub;
  if (s.row < 0 || s.row >= P.P) return false;
  const float v = P.vals[pix * P.K + k];
  s.r2 = 1.0f;
  s.a = v;
  if (P.flags & MR_COMPOSITE_DISTS) {
    if (P.radius && i >= P.nrad) return false;
    const float r = P.radius ? P.radius[i] : P.r0;
    s.r2 = r * r;
    s.a = 1.0f - v / s.r2;
  }
  return true;
}

#define MRP_NORM_EPS 1e-4f

__global__ void __launch_bounds__(MRP_BLOCK) k_composite_fwd(CompositeParams P, float* __restrict__ out) {
  const int64_t pix = (int64_t)blockIdx.x * MRP_BLOCK + threadIdx.x;
  if (pix >= P.npix) return;
  const int K = P.K, C = P.C;
  float* __restrict__ o = out + pix * C;
  if (P.bg && P.idx[pix * K] < 0) {
    for (int c = 0; c < C; ++c) o[c] = P.bg[c];
    return;
  }
  const int64_t sub = P.feat_sub ? P.feat_sub[pix / P.hw] : 0;
  const bool norm = P.flags & MR_COMPOSITE_NORM;
  float den = 1.0f;
  if (norm) {
    float s = 0.0f;
    Slot q;
    for (int k = 0; k < K; ++k)
      if (comp_slot(P, pix, sub, k, q)) s += q.a;
    den = smax(s, MRP_NORM_EPS);
  }
  for (int c0 = 0; c0 < C; c0 += 4) {
    const int nc = min(4, C - c0);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float T = 1.0f;
    Slot q;
    for (int k = 0; k < K; ++k) {
      if (!comp_slot(P, pix, sub, k, q)) continue;
      const float w = norm ? q.a : q.a * T;
      const float* __restrict__ f = P.feats + q.row * C + c0;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < nc) acc[c] += f[c] * w;
      T *= 1.0f - q.a;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < nc) o[c0 + c] = norm ? acc[c] / den : acc[c];
  }
}

// alpha: out = B_0 with B_k = f_k a_k + (1 - a_k) B_{k+1}; d out / d a_k = T_k (f_k - B_{k+1}), T_k = prod_{j<k}(1 - a_j):
// a far-to-near pass leaves sum_c g_c (f_k - B_{k+1}) in gvals[k], a near-to-far pass scales it by T_k (no division
// by 1 - a). norm: out = sum_k f_k a_k / D, D = max(sum a, eps); d / d a_k = g . (f_k - [sum a >= eps] out) / D.
__global__ void __launch_bounds__(MRP_BLOCK) k_composite_bwd(CompositeParams P, const float* __restrict__ gout,
                                                             float* __restrict__ gvals, u64* __restrict__ fix,
                                                             float* __restrict__ rem) {
  const int64_t pix = (int64_t)blockIdx.x * MRP_BLOCK + threadIdx.x;
  if (pix >= P.npix) return;
  const int K = P.K, C = P.C;
  float* __restrict__ gv = gvals + pix * K;
  for (int k = 0; k < K; ++k) gv[k] = 0.0f;
  if (P.bg && P.idx[pix * K] < 0) return;
  const float* __restrict__ g = gout + pix * C;
  const int64_t sub = P.feat_sub ? P.feat_sub[pix / P.hw] : 0;
  const bool norm = P.flags & MR_COMPOSITE_NORM;
  Slot q;
  float s = 0.0f, den = 1.0f;  // norm: the sum of alphas and its clamp
  if (norm) {
    for (int k = 0; k < K; ++k)
      if (comp_slot(P, pix, sub, k, q)) s += q.a;
    den = smax(s, MRP_NORM_EPS);
  }
  for (int c0 = 0; c0 < C; c0 += 4) {
    const int nc = min(4, C - c0);
    // B: alpha: the composite of the slots behind k; norm: the pixel's output (zero under the clamp, where the
    // denominator is a constant), so that f_k - B is formed per channel before anything is divided by D
    float gc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, B[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < nc) gc[c] = g[c0 + c];
    if (norm && s >= MRP_NORM_EPS) {
      for (int k = 0; k < K; ++k) {
        if (!comp_slot(P, pix, sub, k, q)) continue;
        const float* __restrict__ f = P.feats + q.row * C + c0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < nc) B[c] += f[c] * q.a;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) B[c] = B[c] / den;
    }
    for (int k = K - 1; k >= 0; --k) {
      if (!comp_slot(P, pix, sub, k, q)) continue;
      const float* __restrict__ f = P.feats + q.row * C + c0;
      float d = 0.0f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c >= nc) continue;
        d += gc[c] * (f[c] - B[c]);
        if (!norm) B[c] = f[c] * q.a + (1.0f - q.a) * B[c];
      }
      gv[k] += d;
    }
  }
  float T = 1.0f;
  for (int k = 0; k < K; ++k) {
    if (!comp_slot(P, pix, sub, k, q)) continue;
    const float w = norm ? q.a / den : q.a * T;
    const float ga = norm ? gv[k] / den : gv[k] * T;
    gv[k] = (P.flags & MR_COMPOSITE_DISTS) ? -ga / q.r2 : ga;
    for (int c = 0; c < C; ++c) fix_add(fix, rem, q.row * C + c, g[c] * w);
    T *= 1.0f - q.a;
  }
}

int check_raster(const char* who, int64_t N, int64_t total, int32_t H, int32_t W, int32_t K) {
  if (N < 1 || total < 0) return set_err(MR_EINVAL, "%s: N must be >= 1 and total_points >= 0", who);
  if (H < 1 || W < 1 || H > 32768 || W > 32768) return set_err(MR_EINVAL, "%s: image size out of range", who);
  if (K < 1) return set_err(MR_EINVAL, "%s: points_per_pixel must be >= 1", who);
  if (K > MRP_KMAX) return set_err(MR_EUNSUPPORTED, "%s: points_per_pixel > %d is not implemented", who, MRP_KMAX);
  if (total >= 0x7fffffffll) return set_err(MR_EUNSUPPORTED, "%s: more than 2^31 - 1 points", who);
  if (N * (int64_t)H * W >= (1ll << 40) / K) return set_err(MR_EUNSUPPORTED, "%s: N H W K is too large", who);
  return MR_OK;
}

int check_composite(const char* who, int64_t N, int32_t H, int32_t W, int32_t K, int32_t C, int64_t P, int32_t flags) {
  if (N < 1 || H < 1 || W < 1 || K < 1 || C < 1 || P < 0) return set_err(MR_EINVAL, "%s: sizes out of range", who);
  if (flags & ~(MR_COMPOSITE_NORM | MR_COMPOSITE_DISTS)) return set_err(MR_EINVAL, "%s: unknown bits in flags", who);
  if (N * (int64_t)H * W >= (1ll << 40) / (K > C ? K : C) || P >= (1ll << 40) / C)
    return set_err(MR_EUNSUPPORTED, "%s: sizes too large", who);
  return MR_OK;
}

}  // namespace

extern "C" {

int32_t mr_point_raster_chunk(void) { return MRP_CHUNK; }

int32_t mr_rasterize_points(const float* points, const int64_t* first, const int64_t* count, const int64_t* idx_base,
                            int64_t N, int64_t total_points, int32_t H, int32_t W, float radius,
                            const float* radius_per_point, int32_t K, int64_t* idx, float* zbuf, float* dists,
                            void* stream) {
  if (int rc = check_raster("rasterize points", N, total_points, H, W, K)) return rc;
  if (!first || !count || !idx || !zbuf || !dists || (total_points > 0 && !points))
    return set_err(MR_EINVAL, "rasterize points: NULL pointer");
  PointRasterParams P;
  P.pts = points;
  P.first = first;
  P.count = count;
  P.idx_base = idx_base;
  P.radius = radius_per_point;
  P.r0 = radius;
  P.N = N;
  P.total = total_points;
  P.H = H;
  P.W = W;
  P.K = K;
  P.idx = idx;
  P.zbuf = zbuf;
  P.dists = dists;
  const int nw = K <= MRP_K4 ? 4 : 1, mt = nw == 4 ? 16 : 8;
  P.mtx = ceil_div(W, mt);
  P.mty = ceil_div(H, mt);
  const int64_t tiles = N * (int64_t)P.mtx * P.mty;
  const unsigned grid = (unsigned)(tiles < (1ll << 20) ? tiles : (1ll << 20));
  const size_t lds = sizeof(u64) * (size_t)K * 64 * nw + MRP_CHUNK * (sizeof(float4) + sizeof(int));
  return launch(KID_NONE, "k_point_raster", nw == 4 ? k_point_raster<4> : k_point_raster<1>, grid, 64 * nw, lds,
                (hipStream_t)stream, P);
}

size_t mr_rasterize_points_backward_workspace(int64_t total_points) {
  if (total_points < 0 || total_points >= 0x7fffffffll) return 0;
  return carve_rows(nullptr, 3 * total_points).bytes;
}

int32_t mr_rasterize_points_backward(const float* points, const int64_t* first, const int64_t* idx_base, int64_t N,
                                     int64_t total_points, int32_t H, int32_t W, int32_t K, const int64_t* idx,
                                     const float* grad_zbuf, const float* grad_dists, float* grad_points, void* ws,
                                     size_t ws_bytes, void* stream) {
  if (int rc = check_raster("rasterize points backward", N, total_points, H, W, K)) return rc;
  if (total_points == 0) return MR_OK;
  if (!points || !idx || !grad_points || !ws || (idx_base && !first))
    return set_err(MR_EINVAL, "rasterize points backward: NULL pointer");
  const FixRows w = carve_rows(ws, 3 * total_points);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "rasterize points backward workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  if (int rc = memset_async(ws, 0, w.bytes, st)) return rc;
  const int64_t nslots = N * (int64_t)H * W * K;
  if (grad_zbuf || grad_dists)
    if (int rc = launch(KID_NONE, "k_point_raster_bwd", k_point_raster_bwd, ceil_div(nslots, MRP_BLOCK), MRP_BLOCK, 0, st,
                        points, first, idx_base, total_points, nslots, H, W, K, idx, grad_zbuf, grad_dists, w.fix,
                        w.rem))
      return rc;
  return launch(KID_NONE, "k_pr_fix_to_float", k_pr_fix_to_float, ceil_div(3 * total_points, MRP_BLOCK), MRP_BLOCK, 0, st,
                w.fix, w.rem, 3 * total_points, grad_points);
}

int32_t mr_project_points(const float* points, const int64_t* src_first, const int64_t* dst_first,
                          const int64_t* count, int64_t N, int64_t max_count, const float* views, float* out,
                          void* stream) {
  if (N < 1 || N > 65535 || max_count < 0 || max_count >= 0x7fffffffll)
    return set_err(MR_EINVAL, "project points: N must be in [1, 65535] and max_count in [0, 2^31)");
  if (max_count == 0) return MR_OK;
  if (!points || !src_first || !dst_first || !count || !views || !out)
    return set_err(MR_EINVAL, "project points: NULL pointer");
  return launch(KID_NONE, "k_project_points", k_project_points, dim3(ceil_div(max_count, MRP_BLOCK), (unsigned)N),
                MRP_BLOCK, 0, (hipStream_t)stream, points, src_first, dst_first, count, views, out);
}

size_t mr_project_points_backward_workspace(int64_t total_points) {
  return mr_rasterize_points_backward_workspace(total_points);
}

int32_t mr_project_points_backward(const float* points, const int64_t* src_first, const int64_t* dst_first,
                                   const int64_t* count, int64_t N, int64_t total_points, const float* views,
                                   const float* grad_ndc, float* grad_points, float* grad_views, void* ws,
                                   size_t ws_bytes, void* stream) {
  if (N < 1 || total_points < 0 || total_points >= 0x7fffffffll)
    return set_err(MR_EINVAL, "project points backward: N must be >= 1 and total_points in [0, 2^31)");
  if (!src_first || !dst_first || !count || !views || !grad_views || (total_points > 0 && (!points || !grad_ndc || !grad_points || !ws)))
    return set_err(MR_EINVAL, "project points backward: NULL pointer");
  const FixRows w = carve_rows(ws, 3 * total_points);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "project points backward workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  if (total_points > 0)
    if (int rc = memset_async(ws, 0, w.bytes, st)) return rc;
  if (int rc = launch(KID_NONE, "k_project_points_bwd", k_project_points_bwd, (unsigned)N, MRP_BLOCK, 0, st, points,
                      src_first, dst_first, count, views, grad_ndc, w.fix, w.rem, grad_views))
    return rc;
  if (total_points == 0) return MR_OK;
  return launch(KID_NONE, "k_pr_fix_to_float", k_pr_fix_to_float, ceil_div(3 * total_points, MRP_BLOCK), MRP_BLOCK, 0, st,
                w.fix, w.rem, 3 * total_points, grad_points);
}

static CompositeParams composite_params(const int64_t* idx, const float* vals, const float* feats, int64_t N, int32_t H,
                                        int32_t W, int32_t K, int32_t C, int64_t P, int32_t flags, float radius,
                                        const float* radius_per_point, int64_t n_radius, const int64_t* feat_sub,
                                        const float* background) {
  CompositeParams q;
  q.idx = idx;
  q.vals = vals;
  q.feats = feats;
  q.radius = radius_per_point;
  q.feat_sub = feat_sub;
  q.bg = background;
  q.npix = N * (int64_t)H * W;
  q.hw = (int64_t)H * W;
  q.P = P;
  q.nrad = n_radius;
  q.K = K;
  q.C = C;
  q.flags = flags;
  q.r0 = radius;
  return q;
}

int32_t mr_composite_points_forward(const int64_t* idx, const float* vals, const float* feats, int64_t N, int32_t H,
                                    int32_t W, int32_t K, int32_t C, int64_t P, int32_t flags, float radius,
                                    const float* radius_per_point, int64_t n_radius, const int64_t* feat_sub,
                                    const float* background, float* out, void* stream) {
  if (int rc = check_composite("composite points", N, H, W, K, C, P, flags)) return rc;
  if (!idx || !vals || !out || (P > 0 && !feats)) return set_err(MR_EINVAL, "composite points: NULL pointer");
  const CompositeParams q = composite_params(idx, vals, feats, N, H, W, K, C, P, flags, radius, radius_per_point,
                                             n_radius, feat_sub, background);
  return launch(KID_NONE, "k_composite_fwd", k_composite_fwd, ceil_div(q.npix, MRP_BLOCK), MRP_BLOCK, 0,
                (hipStream_t)stream, q, out);
}

size_t mr_composite_points_backward_workspace(int64_t P, int32_t C) {
  if (P < 0 || C < 1 || P >= (1ll << 40) / C) return 0;
  return carve_rows(nullptr, P * C).bytes;
}

int32_t mr_composite_points_backward(const int64_t* idx, const float* vals, const float* feats, int64_t N, int32_t H,
                                     int32_t W, int32_t K, int32_t C, int64_t P, int32_t flags, float radius,
                                     const float* radius_per_point, int64_t n_radius, const int64_t* feat_sub,
                                     const float* background, const float* grad_out, float* grad_vals,
                                     float* grad_feats, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_composite("composite points backward", N, H, W, K, C, P, flags)) return rc;
  if (!idx || !vals || !grad_out || !grad_vals || (P > 0 && (!feats || !grad_feats || !ws)))
    return set_err(MR_EINVAL, "composite points backward: NULL pointer");
  const FixRows w = carve_rows(ws, P * C);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "composite points backward workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  if (int rc = memset_async(ws, 0, w.bytes, st)) return rc;
  const CompositeParams q = composite_params(idx, vals, feats, N, H, W, K, C, P, flags, radius, radius_per_point,
                                             n_radius, feat_sub, background);
  if (int rc = launch(KID_NONE, "k_composite_bwd", k_composite_bwd, ceil_div(q.npix, MRP_BLOCK), MRP_BLOCK, 0, st, q,
                      grad_out, grad_vals, w.fix, w.rem))
    return rc;
  if (P == 0) return MR_OK;
  return launch(KID_NONE, "k_pr_fix_to_float", k_pr_fix_to_float, ceil_div(P * C, MRP_BLOCK), MRP_BLOCK, 0, st, w.fix,
                w.rem, P * C, grad_feats);
}

}  // extern "C"
