// mi355r — What the searches through a point grid (mr_grid.hip's k_knn_grid, mr_points.hip's k_icp_nn_grid,
// mr_normals.hip's k_frames_grid, mr_ballquery.hip's k_ball_query_grid) share, one copy of each: the layout of the grid buffer (GridHead, grid_budget, carve_grid), the head as a search may use it
// (head_dims), a coordinate's cell (cell_axis), the lower bound on the distances beyond the rings (ring_bound), the visit
// of a run of cells (visit_range) and the lane's walk over the cube rings around its query (grid_walk). mr_grid.hip
// states the layout and builds the buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mr_host.h"
#include "mr_cloud.h"
#include "mr_knn.h"

#define MRG_MAXDIM 1024        // cells along one axis (the bound's rounding argument needs <= 2^12)
#define MRG_MAXCELLS (1 << 24) // cells per cloud
#define MRG_MIN_BOUND 0x1p-100f
#define MRG_QBLOCK 64          // threads of the query kernels: one wave

namespace {

struct GridHead {  // 64 bytes
  float lo[3];
  float h, inv_h;
  int32_t g[3];
  int32_t max_count;
  int32_t pad[7];
};

inline int64_t grid_budget(int64_t P) { return P < MRG_MAXCELLS ? P : MRG_MAXCELLS; }

struct GridBuf {
  GridHead* head;
  uint32_t* cell_start;  // (N, budget + 1)
  float4* pts;           // (N, P)
  size_t bytes;
};
inline GridBuf carve_grid(const void* base, int64_t N, int64_t P) {
  GridBuf b;
  Carver c(base);
  b.head = c.take<GridHead>((size_t)N);
  b.cell_start = c.take<uint32_t>((size_t)N * (size_t)(grid_budget(P) + 1));
  b.pts = c.take<float4>((size_t)N * (size_t)P);
  b.bytes = c.off;
  return b;
}

// A coordinate's cell along one axis: clamp(floor((p - lo) * inv_h), 0, g - 1) in float32; a nan lands in cell 0.
__device__ __forceinline__ int cell_axis(float p, float lo, float inv_h, int g) {
  const float u = floorf((p - lo) * inv_h);
  const int c = (int)fminf(fmaxf(u, 0.0f), (float)(g - 1));
  return c < 0 ? 0 : (c > g - 1 ? g - 1 : c);
}

// The head as a search may use it: dims in [1, MRG_MAXDIM] whose product is within the budget, else one cell.
__device__ __forceinline__ void head_dims(const GridHead& H, int64_t budget, int& gx, int& gy, int& gz) {
  gx = H.g[0];
  gy = H.g[1];
  gz = H.g[2];
  const bool ok = gx >= 1 && gy >= 1 && gz >= 1 && gx <= MRG_MAXDIM && gy <= MRG_MAXDIM && gz <= MRG_MAXDIM &&
                  (int64_t)gx * gy * gz <= budget;
  if (!ok) gx = gy = gz = 1;
}

// A lower bound on the float32 distance from a query to every target whose cell lies outside the rings 0 .. r >= 1
// around the query's cell: the rings' cells separate the two by more than r cells along one axis. 0 (never reached)
// where the arithmetic would leave the normal numbers.
template <int NORM> __device__ __forceinline__ float ring_bound(int r, float h) {
  const float rb = ((float)r - 0x1p-6f) * h;
  const float bound = (NORM == 2 ? rb * rb : rb) * (1.0f - 0x1p-18f);
  return bound >= MRG_MIN_BOUND ? bound : 0.0f;
}

// A radius search's key, (index << 32) | float bits of the distance: ascending keys are ascending indices, so the KB
// smallest are the first KB hits in index order, which is ball_query's rule.
__device__ __forceinline__ u64 ball_key(float dist, uint32_t index) {
  return ((u64)index << 32) | (u64)__float_as_uint(dist);
}

// Targets b .. e of the cell order (clamped to the cloud's lt) into the list; returns how many were evaluated. BALL:
// only a target whose distance is strictly below `cap` enters, on ball_key.
template <int NORM, int KB, bool BALL>
__device__ __forceinline__ uint32_t visit_range(const uint32_t* __restrict__ cs, int64_t cb, int64_t ce,
                                                const float4* __restrict__ tp, uint32_t lt, uint32_t last, float qx,
                                                float qy, float qz, float cap, u64 (&L)[KB]) {
  uint32_t b = cs[cb], e = cs[ce];
  b = b < lt ? b : lt;
  e = e < lt ? e : lt;
  for (uint32_t j = b; j < e; ++j) {
    const float4 t = tp[j];
    const uint32_t id = __float_as_uint(t.w);
    if (BALL) {
      const float d = dist3<NORM>(qx, qy, qz, t);
      const u64 key = ball_key(d, id < last ? id : last);
      if (d < cap && key < L[KB - 1]) knn_insert<KB>(L, key);  // false for a nan distance
    } else {
      const u64 key = nn_key(dist3<NORM>(qx, qy, qz, t), id < last ? id : last);
      if (key < L[KB - 1]) knn_insert<KB>(L, key);
    }
  }
  return e > b ? e - b : 0u;
}

// One lane's search of its cloud's grid (dims gx, gy, gz from head_dims, cell size h; cs the cloud's cell_start, tp its
// targets in cell order, lt its length, last = P2 - 1) for the query (qx, qy, qz): the KB smallest keys, ascending, in
// L, which the caller has initialised (a candidate enters on a strictly smaller 64-bit key than L[KB - 1]). The lane
// walks cube rings r = 0, 1, .. around the query's own cell: per (z, y) row of a ring either the whole x run (one
// range of targets) or the run's two end cells. After ring r >= 1 it stops once its K-th distance is strictly below
// ring_bound(r) (a distance that is inf or a nan never is), or, with CAP, once ring_bound(r) > cap: no target beyond
// the rings can then lie within `cap` (ring_bound's 0 never stops it), or when the rings cover the grid. With BALL
// (a radius search: visit_range says what enters) a full list stops nothing, since a later cell may hold a lower index:
// only the CAP stop and the cover end the walk. `seen` gains
// the number of distances evaluated: the caller's counter by reference and not a return value, which cost k_knn_grid
// registers (KB = 8: 128 VGPRs against 69). Every address is clamped: visit_range says how.
template <int NORM, int KB, bool CAP, bool BALL = false>
__device__ __forceinline__ void grid_walk(const GridHead& H, int gx, int gy, int gz, const uint32_t* cs,
                                          const float4* tp, uint32_t lt, uint32_t last, float qx, float qy, float qz,
                                          int K, float cap, u64 (&L)[KB], uint32_t& seen) {
  const int cx = cell_axis(qx, H.lo[0], H.inv_h, gx), cy = cell_axis(qy, H.lo[1], H.inv_h, gy),
            cz = cell_axis(qz, H.lo[2], H.inv_h, gz);
  int cover = cx > gx - 1 - cx ? cx : gx - 1 - cx;  // the ring that reaches the grid's farthest face
  cover = cy > cover ? cy : cover;
  cover = gy - 1 - cy > cover ? gy - 1 - cy : cover;
  cover = cz > cover ? cz : cover;
  cover = gz - 1 - cz > cover ? gz - 1 - cz : cover;
  for (int r = 0;; ++r) {
    const int z0 = cz - r < 0 ? 0 : cz - r, z1 = cz + r > gz - 1 ? gz - 1 : cz + r;
    const int y0 = cy - r < 0 ? 0 : cy - r, y1 = cy + r > gy - 1 ? gy - 1 : cy + r;
    const int x0 = cx - r < 0 ? 0 : cx - r, x1 = cx + r > gx - 1 ? gx - 1 : cx + r;
    for (int z = z0; z <= z1; ++z) {
      for (int y = y0; y <= y1; ++y) {
        const int64_t row = ((int64_t)z * gy + y) * gx;
        const bool face = z == cz - r || z == cz + r || y == cy - r || y == cy + r;
        if (face) {  // the whole run of the row
          seen += visit_range<NORM, KB, BALL>(cs, row + x0, row + x1 + 1, tp, lt, last, qx, qy, qz, cap, L);
        } else {  // the run's interior belongs to nearer rings: its two end cells, where the grid has them
          if (cx - r >= 0)
            seen += visit_range<NORM, KB, BALL>(cs, row + cx - r, row + cx - r + 1, tp, lt, last, qx, qy, qz, cap, L);
          if (cx + r <= gx - 1)
            seen += visit_range<NORM, KB, BALL>(cs, row + cx + r, row + cx + r + 1, tp, lt, last, qx, qy, qz, cap, L);
        }
      }
    }
    if (r >= cover) break;
    if (r >= 1) {
      if (!BALL) {
        u64 worst = L[KB - 1];
#pragma unroll
        for (int j = 0; j < KB - 1; ++j) worst = j == K - 1 ? L[j] : worst;
        if (key_dist(worst) < ring_bound<NORM>(r, H.h)) break;  // an empty slot's distance bits are a nan: false
      }
      if (CAP && ring_bound<NORM>(r, H.h) > cap) break;
    }
  }
}

// Every lane's count of evaluated distances into the counter: one add per wave.
__device__ __forceinline__ void grid_count_visited(uint32_t seen, u64* __restrict__ visited) {
#pragma unroll
  for (int off = MRG_QBLOCK / 2; off > 0; off >>= 1) seen += __shfl_xor(seen, off, MRG_QBLOCK);
  if (threadIdx.x == 0 && seen) atomicAdd(visited, (u64)seen);
}

}  // namespace
