// mi355r — Local coordinate frames of point clouds (PyTorch3D estimate_pointcloud_local_coord_frames /
// estimate_pointcloud_normals, 2 <= K <= 64): mr_point_frames / mr_point_frames_geometry / mr_point_frames_grid /
// mr_symmetric_eig3_host of include/mi355r.h.
//
//   k_frames        k_knn's scan (mr_knn.h's knn_scan) of a cloud against itself: a workgroup owns a tile of queries
//                   (Q per thread) and keeps every query's KB smallest (distance, index) keys ascending in registers,
//                   KB the bucket 8, 16, 32, 64 of K and Q = 4, 2, 1, 1. With splits == 1 the same thread then runs
//                   frames_epilogue on its list: it gathers the K neighbours' coordinates three times (mean of
//                   d_k = p_k - p_i; covariance of d_k - mean; the projections of the sign step), solves the 3x3
//                   with sym_eig3 and stores. No index or neighbour tensor goes to memory on this path.
//   k_frames_merge  only when N * query tiles < 256 (knn_geom's split rule): k_frames writes its K sorted keys per
//                   query and split into the workspace, and one thread per query merges them by key and runs the same
//                   frames_epilogue. The key order is total and the epilogue sums in list order, so the result does
//                   not depend on the splits, bit for bit.
//   k_frames_grid   mr_point_frames_grid: one query per lane walks its cloud's point grid (mr_grid.h's grid_walk) to
//                   the same list and runs the same frames_epilogue: one launch, no workspace, the same bits.
//   sym_eig3       eigenvalues (ascending) and unit eigenvectors of a symmetric 3x3 in float32: the matrix is divided
//                   by the sum of its diagonal's magnitudes (its trace, for a covariance), so the iteration sees the
//                   same numbers at every scale of the cloud; MRF_SWEEPS cyclic Jacobi sweeps, the count fixed; host
//                   and device run the same operations (no contraction, correctly rounded division and square root).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mi355r.h"
#include "mr_host.h"
#include "mr_cloud.h"
#include "mr_knn.h"
#include "mr_grid.h"

#define MRF_MINK 2
#define MRF_MAXK 64
#define MRF_MIN_BUCKET 8
#define MRF_GATHER 8   // neighbours whose loads the scheduler may put in flight together (the rest cost registers)
#define MRF_SWEEPS 8   // cyclic Jacobi sweeps of the 3x3 (three rotations each; a zero off-diagonal is skipped)

namespace {

// One Jacobi rotation in the (P, Q) plane; R is the third axis. A stays symmetric; V's columns take the rotation.
template <int P, int Q, int R>
__host__ __device__ __forceinline__ void jacobi_rotate(float (&A)[3][3], float (&V)[3][3]) {
  const float apq = A[P][Q];
  if (apq == 0.0f) return;
  const float theta = (A[Q][Q] - A[P][P]) / (2.0f * apq);  // +-inf for a tiny apq: t = 0 below
  const float t = (theta < 0.0f ? -1.0f : 1.0f) / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
  const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
  A[P][P] -= t * apq;
  A[Q][Q] += t * apq;
  A[P][Q] = A[Q][P] = 0.0f;
  const float arp = A[R][P], arq = A[R][Q];
  A[R][P] = A[P][R] = c * arp - s * arq;
  A[R][Q] = A[Q][R] = s * arp + c * arq;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float vp = V[i][P], vq = V[i][Q];
    V[i][P] = c * vp - s * vq;
    V[i][Q] = s * vp + c * vq;
  }
}

template <int I, int J> __host__ __device__ __forceinline__ void order_pair(float (&lam)[3], float (&V)[3][3]) {
  if (lam[I] > lam[J]) {
    const float l = lam[I];
    lam[I] = lam[J];
    lam[J] = l;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float v = V[r][I];
      V[r][I] = V[r][J];
      V[r][J] = v;
    }
  }
}

// c: the upper triangle xx, xy, xz, yy, yz, zz. lam ascending, V[:, j] the unit eigenvector of lam[j]. A matrix whose
// diagonal is all zero (a covariance of coincident points) gives lam = 0 and the identity.
__host__ __device__ inline void sym_eig3(const float (&c)[6], float (&lam)[3], float (&V)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0f : 0.0f;
  const float scale = (fabsf(c[0]) + fabsf(c[3])) + fabsf(c[5]);
  if (!(scale > 0.0f)) {
    lam[0] = lam[1] = lam[2] = 0.0f;
    return;
  }
  float A[3][3];
  A[0][0] = c[0] / scale;
  A[1][1] = c[3] / scale;
  A[2][2] = c[5] / scale;
  A[0][1] = A[1][0] = c[1] / scale;
  A[0][2] = A[2][0] = c[2] / scale;
  A[1][2] = A[2][1] = c[4] / scale;
  for (int sweep = 0; sweep < MRF_SWEEPS; ++sweep) {
    jacobi_rotate<0, 1, 2>(A, V);
    jacobi_rotate<0, 2, 1>(A, V);
    jacobi_rotate<1, 2, 0>(A, V);
  }
  lam[0] = A[0][0] * scale;
  lam[1] = A[1][1] * scale;
  lam[2] = A[2][2] * scale;
  order_pair<0, 1>(lam, V);
  order_pair<1, 2>(lam, V);
  order_pair<0, 1>(lam, V);
}

// Column j signed so that its component of largest magnitude is positive; ties go to the lowest axis.
__host__ __device__ __forceinline__ void sign_by_largest(float (&V)[3][3], int j) {
  float big = V[0][j];
  if (fabsf(V[1][j]) > fabsf(big)) big = V[1][j];
  if (fabsf(V[2][j]) > fabsf(big)) big = V[2][j];
  if (big < 0.0f) {
    V[0][j] = -V[0][j];
    V[1][j] = -V[1][j];
    V[2][j] = -V[2][j];
  }
}

// The frame of query (px, py, pz), row `self` of its cloud `pts`, from its ascending neighbour list. ok: the row is
// inside its cloud; a list with fewer than K keys (a cloud shorter than K) is treated like a row outside. Every slot
// is visited with compile-time indices; the slots j >= K load the query itself and add +0.
template <int KB>
__device__ __forceinline__ void frames_epilogue(const u64 (&L)[KB], bool ok, int K, const float* __restrict__ pts,
                                                int64_t self, float px, float py, float pz, int flags,
                                                float* __restrict__ cur, float* __restrict__ frm,
                                                float* __restrict__ cov) {
#pragma unroll
  for (int j = 0; j < KB; ++j)
    if (j == K - 1) ok = ok && L[j] != ~0ull;
  const float inv_k = 1.0f / (float)K;
// Slot j's neighbour minus the query: the loads are unconditional (a slot outside reads the query's own row) and the
// differences selected, so a pass is straight-line code. `fresh` is a zero the compiler cannot see through, new in
// every pass: it would otherwise keep all 3 K differences of the first pass in registers for the next two, beside
// the list (more than the register file at KB = 64).
#define MRF_NEIGHBOUR(j)                                                                        \
  if ((j) % MRF_GATHER == 0) __builtin_amdgcn_sched_barrier(0);                                 \
  const bool in = ok && (j) < K;                                                                \
  const float* __restrict__ nb = pts + 3 * (int64_t)((in ? key_index(L[j]) : (uint32_t)self) + fresh); \
  const float lx = nb[0], ly = nb[1], lz = nb[2];                                               \
  const float dx = in ? lx - px : 0.0f, dy = in ? ly - py : 0.0f, dz = in ? lz - pz : 0.0f
#define MRF_NEW_PASS()  \
  uint32_t fresh = 0u;  \
  asm volatile("" : "+v"(fresh))
  float mx = 0.0f, my = 0.0f, mz = 0.0f;
  {
    MRF_NEW_PASS();
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    MRF_NEIGHBOUR(j);
    mx += dx;
    my += dy;
    mz += dz;
  }
  }
  mx *= inv_k;
  my *= inv_k;
  mz *= inv_k;
  float c[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  {
    MRF_NEW_PASS();
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    MRF_NEIGHBOUR(j);
    const float ex = in ? dx - mx : 0.0f, ey = in ? dy - my : 0.0f, ez = in ? dz - mz : 0.0f;
    c[0] += ex * ex;
    c[1] += ex * ey;
    c[2] += ex * ez;
    c[3] += ey * ey;
    c[4] += ey * ez;
    c[5] += ez * ez;
  }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) c[a] *= inv_k;
  float lam[3], V[3][3];
  sym_eig3(c, lam, V);
  if (flags & MR_FRAMES_DISAMBIGUATE) {
    int pos0 = 0, pos2 = 0;
    MRF_NEW_PASS();
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      MRF_NEIGHBOUR(j);
      const float pr0 = (V[0][0] * dx + V[1][0] * dy) + V[2][0] * dz;
      const float pr2 = (V[0][2] * dx + V[1][2] * dy) + V[2][2] * dz;
      pos0 += (in && pr0 > 0.0f) ? 1 : 0;
      pos2 += (in && pr2 > 0.0f) ? 1 : 0;
    }
    const float s0 = 2 * pos0 < K ? -1.0f : 1.0f, s2 = 2 * pos2 < K ? -1.0f : 1.0f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      V[r][0] *= s0;
      V[r][2] *= s2;
    }
    V[0][1] = V[1][0] * V[2][2] - V[2][0] * V[1][2];  // column 1 = column 0 x column 2
    V[1][1] = V[2][0] * V[0][2] - V[0][0] * V[2][2];
    V[2][1] = V[0][0] * V[1][2] - V[1][0] * V[0][2];
  } else {
    sign_by_largest(V, 0);
    sign_by_largest(V, 1);
    sign_by_largest(V, 2);
  }
#undef MRF_NEW_PASS
#undef MRF_NEIGHBOUR
#pragma unroll
  for (int a = 0; a < 3; ++a) cur[a] = ok ? lam[a] : 0.0f;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int j = 0; j < 3; ++j) frm[3 * r + j] = ok ? V[r][j] : 0.0f;
  if (cov) {
#pragma unroll
    for (int a = 0; a < 6; ++a) cov[a] = ok ? c[a] : 0.0f;
  }
}

// grid (query tiles * splits, N). part != NULL: (N, P, splits, K) keys for k_frames_merge; else the frames themselves.
// The tile prologue and the store of the partial lists stay written out here, beside mr_knn.h's scan_tile and
// knn_store_keys, which k_knn uses: with the helpers KB = 64 ran 4.6 % slower (1 x 20,000, K = 50: 6,944 / 6,992 us
// against 6,680 / 6,643; 300 x 2,000: 13,823 / 13,833 against 13,192 / 13,229) and KB = 16 compiled to 129 VGPRs for
// 128, three waves per SIMD for four (profiles/neighbour_fold_ab.txt, neighbour_fold_codeobj.txt).
template <int KB, int Q>
__global__ void __launch_bounds__(MRN_BLOCK) k_frames(const float* __restrict__ pts, int64_t P,
                                                      const int64_t* __restrict__ lens, int K, int flags, int splits,
                                                      int64_t per, float* __restrict__ cur, float* __restrict__ frm,
                                                      float* __restrict__ cov, u64* __restrict__ part) {
  __shared__ float4 sm[MRN_MAXCHUNK];
  const int64_t n = blockIdx.y;
  const int64_t q0 = ((int64_t)blockIdx.x / splits) * (MRN_BLOCK * Q);
  const int s = (int)((int64_t)blockIdx.x % splits);
  const int64_t len = cloud_len(lens, n, P);
  const float* __restrict__ cloud = pts + 3 * n * P;
  const int64_t tb = (int64_t)s * per;
  int64_t te = tb + per < len ? tb + per : len;
  if (q0 >= len) te = tb;  // no query of this tile is inside its cloud (uniform): nothing to scan

  float qx[Q], qy[Q], qz[Q];
  u64 L[Q][KB];
  scan_load_queries(cloud, q0, len, nullptr, false, qx, qy, qz);
#pragma unroll
  for (int k = 0; k < Q; ++k)
#pragma unroll
    for (int j = 0; j < KB; ++j) L[k][j] = ~0ull;
  knn_scan<2, KB, Q>(sm, cloud, tb, te, qx, qy, qz, L);
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    const int64_t i = q0 + k * MRN_BLOCK + threadIdx.x;
    if (i >= P) continue;
    const int64_t row = n * P + i;
    if (part) {
      u64* __restrict__ o = part + (row * splits + s) * K;
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        if (j < K) o[j] = i < len ? L[k][j] : ~0ull;
      }
    } else {
      frames_epilogue<KB>(L[k], i < len, K, cloud, i, qx[k], qy[k], qz[k], flags, cur + 3 * row, frm + 9 * row,
                          cov ? cov + 6 * row : nullptr);
    }
  }
}

// One thread per row of (N, P): its `splits` ascending lists of K keys -> the K smallest -> the frame.
template <int KB>
__global__ void __launch_bounds__(MRK_TBLOCK) k_frames_merge(const float* __restrict__ pts, int64_t P,
                                                             const int64_t* __restrict__ lens,
                                                             const u64* __restrict__ part, int64_t rows, int K,
                                                             int flags, int splits, float* __restrict__ cur,
                                                             float* __restrict__ frm, float* __restrict__ cov) {
  const int64_t row = (int64_t)blockIdx.x * MRK_TBLOCK + threadIdx.x;
  if (row >= rows) return;
  const int64_t n = row / P, i = row - n * P;
  const bool inside = i < cloud_len(lens, n, P);
  const float* __restrict__ cloud = pts + 3 * n * P;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (inside) {
    px = cloud[3 * i];
    py = cloud[3 * i + 1];
    pz = cloud[3 * i + 2];
  }
  u64 L[KB];
  knn_merge_lists<KB>(part, row, K, splits, L);
  frames_epilogue<KB>(L, inside, K, cloud, i, px, py, pz, flags, cur + 3 * row, frm + 9 * row,
                      cov ? cov + 6 * row : nullptr);
}

// grid (blocks over P, N), one wave a workgroup: k_frames' result through the cloud's own point grid (mr_grid.h). A
// lane's query is entry j of its cloud's cell-ordered targets, so the lanes of a wave walk neighbouring cells (against
// lane = point j: 136 us for 223 at 1 x 20,000, K = 16); its output row is the index stored beside the
// coordinates, clamped as visit_range clamps it. grid_walk leaves the same KB smallest keys as knn_scan: the same
// distance expression, the total key order, the point itself included; frames_epilogue sums in list order, so the
// outputs are those of k_frames bit for bit. Lanes j >= length write the zero rows j. Nothing but the outputs goes to
// memory. A stale grid (other clouds of the same shape) gives wrong frames and, two entries naming one row, may leave
// rows unwritten; every address stays in range, which is all a stale grid is promised.
template <int KB>
__global__ void __launch_bounds__(MRG_QBLOCK) k_frames_grid(const float* __restrict__ pts, int64_t P,
                                                            const int64_t* __restrict__ lens, int64_t budget,
                                                            const GridHead* __restrict__ heads,
                                                            const uint32_t* __restrict__ cell_start,
                                                            const float4* __restrict__ gp, int K, int flags,
                                                            float* __restrict__ cur, float* __restrict__ frm,
                                                            float* __restrict__ cov, u64* __restrict__ visited) {
  const int64_t n = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * MRG_QBLOCK + threadIdx.x;
  const int64_t len = cloud_len(lens, n, P);
  const float* __restrict__ cloud = pts + 3 * n * P;
  const GridHead H = heads[n];
  int gx, gy, gz;
  head_dims(H, budget, gx, gy, gz);
  u64 L[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) L[k] = ~0ull;
  uint32_t seen = 0u;
  const bool inside = j < len;
  int64_t i = j;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (inside) {
    const float4 t = gp[n * P + j];
    const uint32_t id = __float_as_uint(t.w), last = (uint32_t)(P - 1);
    i = id < last ? id : last;
    px = t.x;
    py = t.y;
    pz = t.z;
    grid_walk<2, KB, false>(H, gx, gy, gz, cell_start + n * (budget + 1), gp + n * P, (uint32_t)len, last, px, py, pz,
                            K, 0.0f, L, seen);
  }
  if (j < P) {
    const int64_t row = n * P + i;
    frames_epilogue<KB>(L, inside, K, cloud, i, px, py, pz, flags, cur + 3 * row, frm + 9 * row,
                        cov ? cov + 6 * row : nullptr);
  }
  if (visited) grid_count_visited(seen, visited);
}

int check_frames(const char* who, int64_t N, int64_t P, int32_t K) {
  if (int rc = check_sizes(who, N, P, P)) return rc;
  if (K < MRF_MINK) return set_err(MR_EINVAL, "%s: K must be >= %d", who, MRF_MINK);
  if (K > MRF_MAXK) return set_err(MR_EUNSUPPORTED, "%s: K > %d is not built", who, MRF_MAXK);
  if (P <= K) return set_err(MR_EINVAL, "%s: a cloud needs more than K points (P = %lld, K = %d)", who, (long long)P, K);
  return MR_OK;
}

bool frames_args_ok(int64_t N, int64_t P, int32_t K) {
  return sizes_ok(N, P, P) && K >= MRF_MINK && K <= MRF_MAXK && P > K;
}

}  // namespace

extern "C" {

int32_t mr_point_frames_geometry(int64_t N, int64_t P, int32_t K, int32_t* bucket, int32_t* queries_per_group,
                                 int32_t* splits, int32_t* lds_chunk) {
  if (int rc = check_frames("point frames geometry", N, P, K)) return rc;
  const KnnGeom g = knn_geom(N, P, P, K, MRF_MIN_BUCKET);
  if (bucket) *bucket = g.kb;
  geom_out(g, queries_per_group, splits, lds_chunk);
  return MR_OK;
}

size_t mr_point_frames_workspace(int64_t N, int64_t P, int32_t K) {
  if (!frames_args_ok(N, P, K)) return 0;
  return knn_ws_bytes(N, P, K, knn_geom(N, P, P, K, MRF_MIN_BUCKET));
}

int32_t mr_point_frames(const float* points, int64_t N, int64_t P, const int64_t* lengths, int32_t K, int32_t flags,
                        float* curvatures, float* frames, float* cov, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_frames("point frames", N, P, K)) return rc;
  if (!points || !curvatures || !frames || !ws)
    return set_err(MR_EINVAL, "point frames: points / curvatures / frames / workspace is NULL");
  if (flags & ~MR_FRAMES_DISAMBIGUATE) return set_err(MR_EINVAL, "point frames: unknown flags 0x%x", flags);
  if (ws_bytes < mr_point_frames_workspace(N, P, K)) return set_err(MR_EWORKSPACE, "point frames workspace too small");
  const KnnGeom g = knn_geom(N, P, P, K, MRF_MIN_BUCKET);
  const hipStream_t st = (hipStream_t)stream;
  u64* part = g.splits > 1 ? (u64*)ws : nullptr;
  const dim3 grid((unsigned)(g.qtiles * g.splits), (unsigned)N);
  const int k = K, fl = flags, splits = g.splits;
  int rc;
#define MRF_SCAN(KB, Q)                                                                                            \
  rc = launch(KID_NONE, "k_frames", k_frames<KB, Q>, grid, MRN_BLOCK, 0, st, points, P, lengths, k, fl, splits, g.per, \
              curvatures, frames, cov, part)
  switch (g.kb) {
    case 8: MRF_SCAN(8, 4); break;
    case 16: MRF_SCAN(16, 2); break;
    case 32: MRF_SCAN(32, 1); break;
    default: MRF_SCAN(64, 1); break;
  }
#undef MRF_SCAN
  if (rc || !part) return rc;
  const int64_t rows = N * P;
  const unsigned mg = (unsigned)((rows + MRK_TBLOCK - 1) / MRK_TBLOCK);
#define MRF_MERGE(KB)                                                                                              \
  case KB:                                                                                                         \
    return launch(KID_NONE, "k_frames_merge", k_frames_merge<KB>, mg, MRK_TBLOCK, 0, st, points, P, lengths,      \
                  (const u64*)part, rows, k, fl, splits, curvatures, frames, cov)
  switch (g.kb) {
    MRF_MERGE(8);
    MRF_MERGE(16);
    MRF_MERGE(32);
    default:
    MRF_MERGE(64);
  }
#undef MRF_MERGE
}

size_t mr_point_frames_grid_workspace(int64_t N, int64_t P, int32_t K) {
  if (!frames_args_ok(N, P, K)) return 0;
  return 256;  // nothing is kept between the lanes; never 0, which means "out of range"
}

int32_t mr_point_frames_grid(const float* points, int64_t N, int64_t P, const int64_t* lengths, const void* grid,
                             size_t grid_bytes, int32_t K, int32_t flags, float* curvatures, float* frames, float* cov,
                             uint64_t* visited, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_frames("point frames grid", N, P, K)) return rc;
  if (!points || !curvatures || !frames || !ws || !grid)
    return set_err(MR_EINVAL, "point frames grid: points / curvatures / frames / grid / workspace is NULL");
  if (flags & ~MR_FRAMES_DISAMBIGUATE) return set_err(MR_EINVAL, "point frames grid: unknown flags 0x%x", flags);
  const GridBuf b = carve_grid(grid, N, P);
  if (grid_bytes < b.bytes) return set_err(MR_EWORKSPACE, "point frames grid: grid buffer too small");
  if (ws_bytes < mr_point_frames_grid_workspace(N, P, K))
    return set_err(MR_EWORKSPACE, "point frames grid workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  const int64_t budget = grid_budget(P);
  const dim3 g((unsigned)ceil_div(P, MRG_QBLOCK), (unsigned)N);
  const int k = K, fl = flags;
  int kb = MRF_MIN_BUCKET;
  while (kb < K) kb *= 2;
#define MRF_GRID(KB)                                                                                           \
  case KB:                                                                                                     \
    return launch(KID_NONE, "k_frames_grid", k_frames_grid<KB>, g, MRG_QBLOCK, 0, st, points, P, lengths, budget, \
                  (const GridHead*)b.head, (const uint32_t*)b.cell_start, (const float4*)b.pts, k, fl, curvatures, \
                  frames, cov, (u64*)visited)
  switch (kb) {
    MRF_GRID(8);
    MRF_GRID(16);
    MRF_GRID(32);
    default:
      MRF_GRID(64);
  }
#undef MRF_GRID
}

int32_t mr_symmetric_eig3_host(const float* cov, int64_t M, float* eigenvalues, float* eigenvectors) {
  if (M < 0) return set_err(MR_EINVAL, "symmetric eig3: M must be >= 0");
  if (M > 0 && (!cov || !eigenvalues || !eigenvectors))
    return set_err(MR_EINVAL, "symmetric eig3: cov / eigenvalues / eigenvectors is NULL");
  for (int64_t m = 0; m < M; ++m) {
    float c[6], lam[3], V[3][3];
    for (int a = 0; a < 6; ++a) c[a] = cov[6 * m + a];
    sym_eig3(c, lam, V);
    for (int j = 0; j < 3; ++j) sign_by_largest(V, j);
    for (int a = 0; a < 3; ++a) eigenvalues[3 * m + a] = lam[a];
    for (int r = 0; r < 3; ++r)
      for (int j = 0; j < 3; ++j) eigenvectors[9 * m + 3 * r + j] = V[r][j];
  }
  return MR_OK;
}

}  // extern "C"
