// mi355r — A uniform-grid index over the targets of a neighbour search, and knn_points through it: mr_point_grid_bytes /
// mr_point_grid_build / mr_knn_points_grid / mr_point_grid_describe of include/mi355r.h.
//
// The grid buffer of a batch (N, P), carved from the shapes alone: a 64-byte GridHead per cloud, cell_start
// (N, budget + 1) uint32 and the targets in cell order (N, P) float4 = (x, y, z, bits of the original index). The
// budget of cells per cloud is grid_budget(P). A cell is (z * gy + y) * gx + x, so a run of cells along x is one
// contiguous range of targets.
//
// Build, four launches, nothing read back:
//   k_grid_bounds  one workgroup per cloud: the bounding box of the first L points and whether all of them are finite;
//                  thread 0 picks the cell size and the dims (grid_plan) and writes the head; the workgroup clears the
//                  cloud's cell counters (a kernel and not a memset node: mr_knn.hip's neighbour_backward says why);
//   k_grid_count   one thread per point: an integer atomic on its cell's counter;
//   k_grid_scan    one workgroup per cloud: the exclusive scan of the counters into cell_start (every thread a
//                  contiguous run of cells, the threads' sums scanned in LDS), the counters become the fill cursors,
//                  the largest count goes into the head;
//   k_grid_fill    one thread per point: its place from an integer atomic on its cell's cursor. The order inside a
//                  cell varies from run to run; no result depends on it.
// Query, one launch:
//   k_knn_grid     one query per lane, its KB smallest keys (mr_cloud.h's nn_key) ascending in registers as in k_knn.
//                  The lane walks cube rings r = 0, 1, .. around its own cell: per (z, y) row of a ring either the whole
//                  x run (one range of targets) or the run's two end cells. Candidates arrive in no index order, so one
//                  enters on the full 64-bit key. After ring r >= 1 the lane stops once its K-th distance is strictly
//                  below ring_bound(r), a lower bound on the float32 distance of every target outside the rings
//                  (DESIGN.md §3 "Point grid" has the argument), or when the rings cover the grid. The walk
//                  (grid_walk), the buffer's layout and what else a search needs live in mr_grid.h, which
//                  mr_points.hip's k_icp_nn_grid, mr_normals.hip's k_frames_grid and mr_ballquery.hip's
//                  k_ball_query_grid share.
// Nothing read from the grid buffer is trusted for addressing: dims are clamped and checked against the budget, target
// ranges are clamped to the cloud's length and stored indices to P2 - 1.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "../../include/mi355r.h"
#include "mr_host.h"
#include "mr_cloud.h"
#include "mr_knn.h"
#include "mr_grid.h"

#define MRG_DENSITY 4.0f       // points per cell the cell size aims for in a uniformly filled box
#define MRG_PLAN_STEPS 512     // growth steps of the cell size before a cloud falls back to one cell
#define MRG_MIN_H 0x1p-100f    // below this the cell size is not used: 1 / h and h * h stay normal numbers
#define MRG_BLOCK 256          // threads of the per-point kernels
#define MRG_CBLOCK 1024        // threads of the per-cloud kernels

namespace {

// The build's workspace: the cell counters, then fill cursors, (N, budget). Never 0.
inline size_t grid_build_ws_bytes(int64_t N, int64_t P) {
  Carver c(nullptr);
  c.take<uint32_t>((size_t)N * (size_t)grid_budget(P) + 1);
  return c.off;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }  // false for nan

// The cell size and dims of a cloud of L points in the box lo .. hi (all_finite: every coordinate is), at most
// `limit` >= 1 cells. h aims at MRG_DENSITY points per cell of the box's non-degenerate axes and grows by a quarter
// until the dims fit; a box that is not finite, or one that never fits, is one cell.
__device__ inline void grid_plan(const float (&lo)[3], const float (&hi)[3], bool all_finite, int64_t L, int64_t limit,
                                 GridHead& H) {
  float e[3];
  bool ok = all_finite && L > 0;
  int d = 0;
  float logv = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    e[a] = hi[a] - lo[a];
    ok = ok && finite_f(lo[a]) && finite_f(e[a]) && e[a] >= 0.0f;
    if (e[a] > 0.0f) {
      ++d;
      logv += log2f(e[a]);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    H.lo[a] = ok ? lo[a] : 0.0f;
    H.g[a] = 1;
  }
  H.h = 1.0f;
  H.inv_h = 1.0f;
  H.max_count = 0;
#pragma unroll
  for (int a = 0; a < 7; ++a) H.pad[a] = 0;
  if (!ok || d == 0) return;
  const float want = fmaxf((float)L / MRG_DENSITY, 1.0f);
  float h = exp2f((logv - log2f(want)) / (float)d);
  if (!(h >= MRG_MIN_H)) h = MRG_MIN_H;  // also a nan
  for (int it = 0; it < MRG_PLAN_STEPS && finite_f(h); ++it, h *= 1.25f) {
    const float inv = 1.0f / h;
    int g[3];
    bool fits = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float cells = floorf(e[a] * inv);  // the cell of the farthest point, as cell_axis computes it
      fits = fits && cells < (float)MRG_MAXDIM;
      g[a] = fits ? (int)cells + 1 : 1;
    }
    if (fits && (int64_t)g[0] * g[1] * g[2] <= limit) {
      H.h = h;
      H.inv_h = inv;
#pragma unroll
      for (int a = 0; a < 3; ++a) H.g[a] = g[a];
      return;
    }
  }
}

// grid (N), MRG_CBLOCK threads. cnt: the cloud's `budget` counters.
__global__ void __launch_bounds__(MRG_CBLOCK) k_grid_bounds(const float* __restrict__ p, int64_t P,
                                                            const int64_t* __restrict__ lengths, int64_t budget,
                                                            GridHead* __restrict__ heads, uint32_t* __restrict__ cnt) {
  __shared__ float sm[7][MRG_CBLOCK];
  __shared__ int64_t s_cells;
  const int64_t n = blockIdx.x;
  const int64_t L = cloud_len(lengths, n, P);
  const float* __restrict__ q = p + 3 * n * P;
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  float bad = 0.0f;
  for (int64_t i = threadIdx.x; i < L; i += MRG_CBLOCK) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = q[3 * i + a];
      if (!finite_f(v)) bad = 1.0f;
      lo[a] = fminf(lo[a], v);
      hi[a] = fmaxf(hi[a], v);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    sm[a][threadIdx.x] = lo[a];
    sm[3 + a][threadIdx.x] = hi[a];
  }
  sm[6][threadIdx.x] = bad;
  __syncthreads();
  for (int s = MRG_CBLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        sm[a][threadIdx.x] = fminf(sm[a][threadIdx.x], sm[a][threadIdx.x + s]);
        sm[3 + a][threadIdx.x] = fmaxf(sm[3 + a][threadIdx.x], sm[3 + a][threadIdx.x + s]);
      }
      sm[6][threadIdx.x] = fmaxf(sm[6][threadIdx.x], sm[6][threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float blo[3] = {sm[0][0], sm[1][0], sm[2][0]}, bhi[3] = {sm[3][0], sm[4][0], sm[5][0]};
    GridHead H;
    const int64_t limit = L < 1 ? 1 : (L < budget ? L : budget);
    grid_plan(blo, bhi, sm[6][0] == 0.0f, L, limit, H);
    heads[n] = H;
    s_cells = (int64_t)H.g[0] * H.g[1] * H.g[2];
  }
  __syncthreads();
  const int64_t cells = s_cells;  // <= limit <= budget
  uint32_t* __restrict__ c = cnt + n * budget;
  for (int64_t i = threadIdx.x; i < cells; i += MRG_CBLOCK) c[i] = 0u;
}

// The cell of point i of cloud n, from the head the build wrote.
__device__ __forceinline__ int64_t point_cell(const GridHead& H, int gx, int gy, int gz, float x, float y, float z) {
  const int cx = cell_axis(x, H.lo[0], H.inv_h, gx), cy = cell_axis(y, H.lo[1], H.inv_h, gy),
            cz = cell_axis(z, H.lo[2], H.inv_h, gz);
  return ((int64_t)cz * gy + cy) * gx + cx;
}

// grid (blocks over P, N). FILL = false: count the cell's points; true: place the point at the cell's cursor.
template <bool FILL>
__global__ void __launch_bounds__(MRG_BLOCK) k_grid_points(const float* __restrict__ p, int64_t P,
                                                           const int64_t* __restrict__ lengths, int64_t budget,
                                                           const GridHead* __restrict__ heads,
                                                           uint32_t* __restrict__ cnt, float4* __restrict__ pts) {
  const int64_t n = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * MRG_BLOCK + threadIdx.x;
  const int64_t L = cloud_len(lengths, n, P);
  if (i >= L) return;
  const GridHead H = heads[n];
  int gx, gy, gz;
  head_dims(H, budget, gx, gy, gz);
  const float* __restrict__ q = p + 3 * (n * P + i);
  const float x = q[0], y = q[1], z = q[2];
  uint32_t* __restrict__ c = cnt + n * budget + point_cell(H, gx, gy, gz, x, y, z);
  if (!FILL) {
    atomicAdd(c, 1u);
  } else {
    const int64_t at = (int64_t)atomicAdd(c, 1u);
    if (at < L) pts[n * P + at] = make_float4(x, y, z, __uint_as_float((uint32_t)i));
  }
}

// grid (N), MRG_CBLOCK threads: cell_start[c] = the points in cells below c, cell_start[cells] = all of them; the
// counters become the cursors of the fill.
__global__ void __launch_bounds__(MRG_CBLOCK) k_grid_scan(int64_t budget, GridHead* __restrict__ heads,
                                                          uint32_t* __restrict__ cnt,
                                                          uint32_t* __restrict__ cell_start) {
  __shared__ uint32_t sum[MRG_CBLOCK];
  __shared__ uint32_t big[MRG_CBLOCK];
  const int64_t n = blockIdx.x;
  int gx, gy, gz;
  head_dims(heads[n], budget, gx, gy, gz);
  const int64_t cells = (int64_t)gx * gy * gz;
  const int64_t per = (cells + MRG_CBLOCK - 1) / MRG_CBLOCK;
  const int64_t b = (int64_t)threadIdx.x * per < cells ? (int64_t)threadIdx.x * per : cells;
  const int64_t e = b + per < cells ? b + per : cells;
  uint32_t* __restrict__ c = cnt + n * budget;
  uint32_t* __restrict__ cs = cell_start + n * (budget + 1);
  uint32_t mine = 0u, most = 0u;
#pragma unroll 4
  for (int64_t i = b; i < e; ++i) {
    const uint32_t v = c[i];
    mine += v;
    most = v > most ? v : most;
  }
  sum[threadIdx.x] = mine;
  big[threadIdx.x] = most;
  __syncthreads();
  for (int off = 1; off < MRG_CBLOCK; off <<= 1) {  // inclusive scan of the threads' sums, running maximum beside it
    const bool has = (int)threadIdx.x >= off;
    const uint32_t v = has ? sum[threadIdx.x - off] : 0u;
    const uint32_t m = has ? big[threadIdx.x - off] : 0u;
    __syncthreads();
    sum[threadIdx.x] += v;
    big[threadIdx.x] = m > big[threadIdx.x] ? m : big[threadIdx.x];
    __syncthreads();
  }
  uint32_t run = sum[threadIdx.x] - mine;
  for (int64_t i = b; i < e; ++i) {
    const uint32_t v = c[i];
    cs[i] = run;
    c[i] = run;
    run += v;
  }
  if (threadIdx.x == MRG_CBLOCK - 1) {
    cs[cells] = sum[MRG_CBLOCK - 1];
    heads[n].max_count = (int32_t)big[MRG_CBLOCK - 1];
  }
}

// grid (blocks over P1, N), one wave a workgroup.
template <int NORM, int KB>
__global__ void __launch_bounds__(MRG_QBLOCK) k_knn_grid(const float* __restrict__ p1, int64_t P1, int64_t P2,
                                                         const int64_t* __restrict__ l1,
                                                         const int64_t* __restrict__ l2, int64_t budget,
                                                         const GridHead* __restrict__ heads,
                                                         const uint32_t* __restrict__ cell_start,
                                                         const float4* __restrict__ pts, int K,
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
    grid_walk<NORM, KB, false>(H, gx, gy, gz, cell_start + n * (budget + 1), pts + n * P2, lt,
                                      (uint32_t)(P2 - 1), q[0], q[1], q[2], K, 0.0f, L, seen);
  }
  if (i < P1) knn_store<KB>(L, i < lq, K, dists + (n * P1 + i) * K, idx + (n * P1 + i) * K);
  if (visited) grid_count_visited(seen, visited);
}

int check_grid_shape(const char* who, int64_t N, int64_t P) {
  if (N < 1 || P < 1) return set_err(MR_EINVAL, "%s: N and P must be >= 1", who);
  if (!sizes_ok(N, 1, P))
    return set_err(MR_EUNSUPPORTED, "%s: more than 65535 clouds or clouds too large for 32-bit point ids", who);
  return MR_OK;
}

}  // namespace

extern "C" {

size_t mr_point_grid_bytes(int64_t N, int64_t P) {
  if (!sizes_ok(N, 1, P)) return 0;
  return carve_grid(nullptr, N, P).bytes;
}

size_t mr_point_grid_build_workspace(int64_t N, int64_t P) {
  if (!sizes_ok(N, 1, P)) return 0;
  return grid_build_ws_bytes(N, P);
}

int32_t mr_point_grid_build(const float* p, int64_t N, int64_t P, const int64_t* lengths, void* grid, size_t grid_bytes,
                            void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_grid_shape("point grid build", N, P)) return rc;
  if (!p || !grid || !ws) return set_err(MR_EINVAL, "point grid build: points / grid / workspace is NULL");
  const GridBuf b = carve_grid(grid, N, P);
  if (grid_bytes < b.bytes) return set_err(MR_EWORKSPACE, "point grid build: grid buffer too small");
  if (ws_bytes < grid_build_ws_bytes(N, P)) return set_err(MR_EWORKSPACE, "point grid build workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  const int64_t budget = grid_budget(P);
  uint32_t* cnt = (uint32_t*)ws;
  const dim3 per_point((unsigned)ceil_div(P, MRG_BLOCK), (unsigned)N);
  if (int rc = launch(KID_NONE, "k_grid_bounds", k_grid_bounds, (unsigned)N, MRG_CBLOCK, 0, st, p, P, lengths, budget,
                      b.head, cnt))
    return rc;
  if (int rc = launch(KID_NONE, "k_grid_count", k_grid_points<false>, per_point, MRG_BLOCK, 0, st, p, P, lengths, budget,
                      (const GridHead*)b.head, cnt, b.pts))
    return rc;
  if (int rc = launch(KID_NONE, "k_grid_scan", k_grid_scan, (unsigned)N, MRG_CBLOCK, 0, st, budget, b.head, cnt,
                      b.cell_start))
    return rc;
  return launch(KID_NONE, "k_grid_fill", k_grid_points<true>, per_point, MRG_BLOCK, 0, st, p, P, lengths, budget,
                (const GridHead*)b.head, cnt, b.pts);
}

size_t mr_knn_points_grid_workspace(int64_t N, int64_t P1, int64_t P2, int32_t K) {
  if (!sizes_ok(N, P1, P2) || K < 1 || K > MRK_MAXK) return 0;
  return 256;  // nothing is kept between the lanes; never 0, which means "out of range"
}

int32_t mr_knn_points_grid(const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2, const int64_t* lengths1,
                           const int64_t* lengths2, const void* grid, size_t grid_bytes, int32_t norm, int32_t K,
                           float* dists, int32_t* idx, uint64_t* visited, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_knn("knn points grid", p1, p2, N, P1, P2, norm, K)) return rc;
  if (!dists || !idx || !ws || !grid) return set_err(MR_EINVAL, "knn points grid: dists / idx / grid / workspace is NULL");
  const GridBuf b = carve_grid(grid, N, P2);
  if (grid_bytes < b.bytes) return set_err(MR_EWORKSPACE, "knn points grid: grid buffer too small");
  if (ws_bytes < mr_knn_points_grid_workspace(N, P1, P2, K))
    return set_err(MR_EWORKSPACE, "knn points grid workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  const int64_t budget = grid_budget(P2);
  const dim3 g((unsigned)ceil_div(P1, MRG_QBLOCK), (unsigned)N);
  const int k = K;
  int kb = 1;
  while (kb < K) kb *= 2;
#define MRG_SEARCH(NORM, KB)                                                                                       \
  case KB:                                                                                                         \
    return launch(KID_NONE, "k_knn_grid", k_knn_grid<NORM, KB>, g, MRG_QBLOCK, 0, st, p1, P1, P2, lengths1, lengths2, \
                  budget, (const GridHead*)b.head, (const uint32_t*)b.cell_start, (const float4*)b.pts, k, dists, idx,  \
                  (u64*)visited)
#define MRG_SEARCH_K(NORM) \
  switch (kb) {            \
    MRG_SEARCH(NORM, 1);   \
    MRG_SEARCH(NORM, 2);   \
    MRG_SEARCH(NORM, 4);   \
    MRG_SEARCH(NORM, 8);   \
    MRG_SEARCH(NORM, 16);  \
    default:               \
      MRG_SEARCH(NORM, 32); \
  }
  if (norm == 2) {
    MRG_SEARCH_K(2)
  }
  MRG_SEARCH_K(1)
#undef MRG_SEARCH_K
#undef MRG_SEARCH
}

int32_t mr_point_grid_describe(const void* grid, int64_t N, int64_t P, int32_t* dims, float* origin_cell,
                               int32_t* max_cell_count, void* stream) {
  if (int rc = check_grid_shape("point grid describe", N, P)) return rc;
  if (!grid) return set_err(MR_EINVAL, "point grid describe: grid is NULL");
  const hipStream_t st = (hipStream_t)stream;
  GridHead* host = (GridHead*)malloc(sizeof(GridHead) * (size_t)N);
  if (!host) return set_err(MR_EINVAL, "point grid describe: out of host memory");
  const bool ok = hipMemcpyAsync(host, carve_grid(grid, N, P).head, sizeof(GridHead) * (size_t)N, hipMemcpyDeviceToHost,
                                 st) == hipSuccess &&
                  hipStreamSynchronize(st) == hipSuccess;
  for (int64_t n = 0; ok && n < N; ++n) {
    for (int a = 0; a < 3; ++a) {
      if (dims) dims[3 * n + a] = host[n].g[a];
      if (origin_cell) origin_cell[4 * n + a] = host[n].lo[a];
    }
    if (origin_cell) origin_cell[4 * n + 3] = host[n].h;
    if (max_cell_count) max_cell_count[n] = host[n].max_count;
  }
  free(host);
  return ok ? MR_OK : set_err(MR_ELAUNCH, "point grid describe: head copy failed");
}

}  // extern "C"
