// mi355r — ICP of point clouds onto mesh surfaces (iterative_closest_point_to_mesh): mr_icp_mesh_* of
// include/mi355r.h, a third estimator on the device-side loop of mr_icp_iterate. A translation unit of its own over
// mr_tri.h (the point-to-triangle pair function and the triangle record) and mr_icp.h (the loop's workspace and status
// words, the float64 Gauss-Newton step); mr_icp_init and mr_icp_transform of mr_points.hip are used as they are.
//
//   k_icpm_prepare  once per registration: every packed face -> its tri_make record, 7 float4 in tri_stage's layout,
//                   into the workspace. The mesh does not change while the loop runs.
//   k_icpm_scan     k_pm_nn's point -> face direction with the cloud's transform applied to the queries in registers
//                   (as k_icp_nn): grid (query tile x face chunk, cloud); a workgroup stages its chunk of records with
//                   coalesced float4 loads, a thread keeps 2 points; chunks merge with a 64-bit atomicMin on nn_key.
//   k_icpm_close    k_icp_plane_moments' tiling: key -> face, key reset; the winner's pair again with pair_dist<true>
//                   for the closest point q and the distance function's gradient direction n (tri_closest), validity,
//                   q and n into the workspace (row i pairs with row i), and the tile's float64 sums of the normal
//                   equations (plane_accum, the point-to-plane step's own code).
//   k_icp_plane_solve / k_icp_plane_status   as the point-to-plane estimator launches them, over q and n.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mi355r.h"
#include "mr_common.h"
#include "mr_host.h"
#include "mr_cloud.h"
#include "mr_tri.h"
#include "mr_icp.h"

#define ICM_BLOCK 256                    // threads of the scan (four waves)
#define ICM_Q 2                          // points per thread of the scan
#define ICM_PTILE (ICM_BLOCK * ICM_Q)    // points per workgroup of the scan
#define ICM_MAXCHUNK 256                 // triangle records staged per workgroup at most (28 KiB of LDS)
#define ICM_MINCHUNK 32
// Workgroups of one scan launch the face chunk aims for (N clouds x query tiles x chunks). Many short workgroups:
// 300 scans of 100-400 points against 5,856 faces take 259 ms per 100 iterations at 32,768 or 131,072 (chunks of 64
// or 32 faces) against 267-269 ms at 2,048 or 8,192 (256 or 224), and one 20,000-point scan 2.12 ms per 5 iterations
// at 8,192 and above (chunks of 32) against 2.49 ms at 2,048 (128): DESIGN.md §3, ICP onto mesh surfaces.
#ifndef ICM_WANT_GROUPS
#define ICM_WANT_GROUPS 32768
#endif

namespace {

struct ICMGeom {
  int chunk;       // faces per workgroup
  int64_t nchunk;  // chunks of the largest mesh
  int64_t groups;  // workgroups per cloud
};

ICMGeom icm_geom(int64_t N, int64_t P1, int64_t max_faces) {
  ICMGeom g;
  const int64_t qtiles = (P1 + ICM_PTILE - 1) / ICM_PTILE;
  int64_t want = ICM_WANT_GROUPS / (N * (qtiles > 1 ? qtiles : 1));
  if (want < 1) want = 1;
  int64_t c = ((max_faces + want - 1) / want + ICM_MINCHUNK - 1) / ICM_MINCHUNK * ICM_MINCHUNK;
  if (c < ICM_MINCHUNK) c = ICM_MINCHUNK;
  if (c > ICM_MAXCHUNK) c = ICM_MAXCHUNK;
  g.chunk = (int)c;
  g.nchunk = (max_faces + c - 1) / c;
  g.groups = qtiles * g.nchunk;
  return g;
}

struct IcpMeshWS {
  IcpPlaneWS plane;  // mr_icp_init's and the point-to-plane step's layout come first
  float4* rec;       // (T, MPM_REC) the packed faces' records
  float* q;          // (N, P1, 3) this iteration's closest points
  float* nrm;        // (N, P1, 3) and gradient directions
  size_t bytes;
};
IcpMeshWS carve_icp_mesh(void* base, int64_t N, int64_t P1, int64_t T) {
  IcpMeshWS w;
  w.plane = carve_icp_plane(base, N, P1);
  Carver c(base, w.plane.bytes);
  w.rec = c.take<float4>((size_t)(T * MPM_REC));
  w.q = c.take<float>((size_t)(3 * N * P1));
  w.nrm = c.take<float>((size_t)(3 * N * P1));
  w.bytes = c.off;
  return w;
}

__global__ void __launch_bounds__(MRR_BLOCK) k_icpm_prepare(const float* __restrict__ verts, int64_t V,
                                                            const int32_t* __restrict__ faces, int64_t T,
                                                            float min_area, float4* __restrict__ rec) {
  const int64_t f = (int64_t)blockIdx.x * MRR_BLOCK + threadIdx.x;
  if (f >= T) return;
  int ia, ib, ic;
  tri_stage(rec + MPM_REC * f, tri_load(verts, V, faces, min_area, f, ia, ib, ic));
}

// Source point i of cloud n under the cloud's transform tr (NULL: as it is).
MR_DEV void icm_point(const float* __restrict__ x, int64_t P1, int64_t n, int64_t i, const float* __restrict__ tr,
                      float (&p)[3]) {
  const float* __restrict__ s = x + 3 * (n * P1 + i);
  p[0] = s[0];
  p[1] = s[1];
  p[2] = s[2];
  if (tr) sim_apply(tr, p[0], p[1], p[2], p[0], p[1], p[2]);
}

// grid (groups, N). rts NULL: the points as they are. status NULL: always runs.
__global__ void __launch_bounds__(ICM_BLOCK) k_icpm_scan(const float* __restrict__ x, int64_t P1,
                                                         const int64_t* __restrict__ xl, const float* __restrict__ rts,
                                                         const float4* __restrict__ rec, int64_t T,
                                                         const int64_t* __restrict__ ff, const int64_t* __restrict__ fc,
                                                         ICMGeom g, const int32_t* __restrict__ status, int max_iter,
                                                         u64* __restrict__ key) {
  __shared__ float4 sm[ICM_MAXCHUNK * MPM_REC];
  if (icp_idle(status, max_iter)) return;
  if ((int64_t)blockIdx.x >= g.groups) return;
  const int64_t n = blockIdx.y;
  const int64_t lq = cloud_len(xl, n, P1);
  int64_t f0, lf;
  range_of(ff, fc, n, T, f0, lf);
  const int64_t q0 = ((int64_t)blockIdx.x / g.nchunk) * ICM_PTILE;
  const int64_t t0 = ((int64_t)blockIdx.x % g.nchunk) * g.chunk;
  if (q0 >= lq || t0 >= lf) return;  // uniform over the workgroup
  const int cnt = (int)((lf - t0 < g.chunk) ? lf - t0 : g.chunk);
  const float4* __restrict__ src = rec + MPM_REC * (f0 + t0);
  for (int j = threadIdx.x; j < cnt * MPM_REC; j += ICM_BLOCK) sm[j] = src[j];
  __syncthreads();
  const float* __restrict__ tr = rts ? rts + n * MRI_RTS : nullptr;
  float p[ICM_Q][3], best[ICM_Q];
  int bi[ICM_Q];
#pragma unroll
  for (int k = 0; k < ICM_Q; ++k) {
    const int64_t i = q0 + k * ICM_BLOCK + threadIdx.x;
    p[k][0] = p[k][1] = p[k][2] = 0.0f;
    if (i < lq) icm_point(x, P1, n, i, tr, p[k]);
    best[k] = __builtin_inff();
    bi[k] = -1;
  }
  tri_scan<ICM_Q>(sm, cnt, p, best, bi);
#pragma unroll
  for (int k = 0; k < ICM_Q; ++k) {
    const int64_t i = q0 + k * ICM_BLOCK + threadIdx.x;
    if (i < lq && bi[k] >= 0) atomicMin(&key[n * P1 + i], nn_key(best[k], (uint32_t)(t0 + bi[k])));
  }
}

// grid (nblk, N), a tile of source points. Decodes key -> (distance, face) and sets the key back to all-ones. Every
// row i < P1 of q / nrm is written (zeros without a face); idx[i] = i for a valid pair (a face, and the distance
// <= max_dist2 or max_dist2 = +inf), else -1; dist / face (each may be NULL) get the distance and the face's index
// within the mesh, 0 / -1 without one. pmom != NULL: the tile's sums of the normal equations about c, and workgroup
// 0 of a cloud copies the transform to prev for k_icp_plane_solve.
__global__ void __launch_bounds__(MRR_BLOCK) k_icpm_close(
    const float* __restrict__ x, int64_t P1, const int64_t* __restrict__ xl, const double* __restrict__ xc,
    const float* __restrict__ rts, const float4* __restrict__ rec, int64_t T, const int64_t* __restrict__ ff,
    const int64_t* __restrict__ fc, float max_dist2, const int32_t* __restrict__ status, int max_iter,
    u64* __restrict__ key, int32_t* __restrict__ idx, float* __restrict__ prev, double* __restrict__ pmom, int64_t nblk,
    float* __restrict__ qout, float* __restrict__ nout, float* __restrict__ dist, int32_t* __restrict__ face) {
  __shared__ double sm[4 * MRI_PMOM];
  if (icp_idle(status, max_iter)) return;
  const int64_t n = blockIdx.y;
  const int64_t lx = cloud_len(xl, n, P1);
  int64_t f0, lf;
  range_of(ff, fc, n, T, f0, lf);
  const float* __restrict__ tr = rts ? rts + n * MRI_RTS : nullptr;
  double c[3] = {0.0, 0.0, 0.0};
  if (pmom) {  // uniform
    if (blockIdx.x == 0 && threadIdx.x < MRI_RTS) prev[n * MRI_RTS + threadIdx.x] = tr[threadIdx.x];
    plane_centre(xc + n * MRI_XC, tr, c);
  }
  const bool every = max_dist2 == __builtin_inff();
  double a[MRI_PMOM];
#pragma unroll
  for (int k = 0; k < MRI_PMOM; ++k) a[k] = 0.0;
#pragma unroll
  for (int k = 0; k < MRR_PER; ++k) {
    const int64_t i = (int64_t)blockIdx.x * MRR_TILE + k * MRR_BLOCK + threadIdx.x;
    if (i >= P1) continue;
    float p[3], q[3] = {0.0f, 0.0f, 0.0f}, nn[3] = {0.0f, 0.0f, 0.0f}, d = 0.0f;
    int64_t j = -1;
    if (i < lx) {
      const u64 kk = key[n * P1 + i];
      key[n * P1 + i] = ~0ull;
      j = (int64_t)key_index(kk);
      if (kk == ~0ull || j >= lf) j = -1;  // no face: the scan left the key untouched
    }
    bool valid = false;
    if (j >= 0) {
      const Tri t = tri_staged<false>(rec + MPM_REC * (f0 + j));
      icm_point(x, P1, n, i, tr, p);
      d = tri_closest(p, t, q, nn);
      valid = every || d <= max_dist2;
    }
    const int64_t o = n * P1 + i;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      qout[3 * o + e] = q[e];
      nout[3 * o + e] = nn[e];
    }
    idx[o] = valid ? (int32_t)i : -1;
    if (dist) dist[o] = d;
    if (face) face[o] = (int32_t)j;
    if (valid && pmom) plane_accum(p[0], p[1], p[2], q, nn, c, a);
  }
  if (pmom) plane_store(a, sm, pmom, n, nblk);
}

int check_icm(const char* who, int64_t N, int64_t P1, int64_t T, const int64_t* ff, const int64_t* fc,
              int64_t max_faces) {
  if (int rc = check_sizes(who, N, P1, 1)) return rc;
  if (T < 0) return set_err(MR_EINVAL, "%s: T must be >= 0", who);
  if (T >= 0x7fffffffll / 3) return set_err(MR_EUNSUPPORTED, "%s: a batch too large for 32-bit face ids", who);
  if (max_faces < 0 || max_faces > T) return set_err(MR_EINVAL, "%s: max_faces outside [0, T]", who);
  if (!ff || !fc) return set_err(MR_EINVAL, "%s: faces_first / faces_count is NULL", who);
  return MR_OK;
}

}  // namespace

extern "C" {

size_t mr_icp_mesh_workspace(int64_t N, int64_t P1, int64_t T) {
  if (!sizes_ok(N, P1, 1) || T < 0 || T >= 0x7fffffffll / 3) return 0;
  return carve_icp_mesh(nullptr, N, P1, T).bytes;
}

int32_t mr_icp_mesh_geometry(int64_t N, int64_t P1, int64_t max_faces, int32_t* chunk, int32_t* min_chunk,
                             int32_t* max_chunk, int64_t* groups) {
  if (int rc = check_sizes("icp mesh geometry", N, P1, 1)) return rc;
  if (max_faces < 0 || max_faces >= 0x7fffffffll / 3) return set_err(MR_EINVAL, "icp mesh geometry: max_faces out of range");
  const ICMGeom g = icm_geom(N, P1, max_faces);
  if (chunk) *chunk = g.chunk;
  if (min_chunk) *min_chunk = ICM_MINCHUNK;
  if (max_chunk) *max_chunk = ICM_MAXCHUNK;
  if (groups) *groups = g.groups;
  return MR_OK;
}

int32_t mr_icp_mesh_prepare(const float* verts, int64_t V, const int32_t* faces, int64_t T, const int64_t* faces_first,
                            const int64_t* faces_count, int64_t max_faces, int64_t N, int64_t P1,
                            float min_triangle_area, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_icm("icp mesh prepare", N, P1, T, faces_first, faces_count, max_faces)) return rc;
  if (V < 0 || V >= 0x7fffffffll / 3) return set_err(MR_EINVAL, "icp mesh prepare: V out of range");
  if (!(min_triangle_area >= 0.0f)) return set_err(MR_EINVAL, "icp mesh prepare: min_triangle_area must be >= 0");
  if (T > 0 && (!faces || !verts)) return set_err(MR_EINVAL, "icp mesh prepare: verts / faces is NULL");
  if (!ws) return set_err(MR_EINVAL, "icp mesh prepare: the workspace is NULL");
  const IcpMeshWS w = carve_icp_mesh(ws, N, P1, T);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "icp mesh workspace too small");
  if (T == 0) return MR_OK;
  return launch(KID_NONE, "k_icpm_prepare", k_icpm_prepare, (unsigned)ceil_div(T, MRR_BLOCK), MRR_BLOCK, 0,
                (hipStream_t)stream, verts, V, faces, T, min_triangle_area, w.rec);
}

int32_t mr_icp_mesh_iterate(const float* x, int64_t N, int64_t P1, const int64_t* x_lengths, int64_t T,
                            const int64_t* faces_first, const int64_t* faces_count, int64_t max_faces, float max_dist2,
                            float relative_rmse_thr, int32_t max_iterations, int32_t iterations, float* rts,
                            float* history, float* rmse, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_icm("icp mesh", N, P1, T, faces_first, faces_count, max_faces)) return rc;
  if (!(max_dist2 >= 0.0f)) return set_err(MR_EINVAL, "icp mesh: max_dist2 must be >= 0 (+inf: no limit)");
  if (max_iterations < 1 || iterations < 0 || (int64_t)max_iterations * N > (1ll << 40) / MRI_RTS)
    return set_err(MR_EINVAL, "icp mesh: max_iterations must be >= 1 (and the history addressable), iterations >= 0");
  if (!x || !rts || !history || !rmse || !status || !ws) return set_err(MR_EINVAL, "icp mesh: NULL pointer");
  const IcpMeshWS w = carve_icp_mesh(ws, N, P1, T);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "icp mesh workspace too small");
  const ICMGeom g = icm_geom(N, P1, max_faces);
  if (g.groups > 0x7fffffffll) return set_err(MR_EUNSUPPORTED, "icp mesh: P1 * T is too large for one launch");
  const hipStream_t st = (hipStream_t)stream;
  const IcpWS& c = w.plane.icp;
  const dim3 gn((unsigned)g.groups, (unsigned)N), gt((unsigned)c.nblk, (unsigned)N);
  for (int it = 0; it < iterations; ++it) {
    if (g.groups > 0)
      if (int rc = launch(KID_NONE, "k_icpm_scan", k_icpm_scan, gn, ICM_BLOCK, 0, st, x, P1, x_lengths, (const float*)rts,
                          (const float4*)w.rec, T, faces_first, faces_count, g, (const int32_t*)status, max_iterations,
                          c.key))
        return rc;
    if (int rc = launch(KID_NONE, "k_icpm_close", k_icpm_close, gt, MRR_BLOCK, 0, st, x, P1, x_lengths,
                        (const double*)c.xc, (const float*)rts, (const float4*)w.rec, T, faces_first, faces_count,
                        max_dist2, (const int32_t*)status, max_iterations, c.key, c.idx, w.plane.prev, w.plane.pmom,
                        c.nblk, w.q, w.nrm, (float*)nullptr, (int32_t*)nullptr))
      return rc;
    if (int rc = launch(KID_NONE, "k_icp_plane_solve", k_icp_plane_solve, gt, MRR_BLOCK, 0, st, x, (const float*)w.q,
                        (const float*)w.nrm, N, P1, P1, x_lengths, (const double*)c.xc, (const double*)w.plane.pmom,
                        c.nblk, (const int32_t*)c.idx, (const float*)w.plane.prev, (const int32_t*)status,
                        max_iterations, rts, history, w.plane.cnt, c.res))
      return rc;
    if (int rc = launch(KID_NONE, "k_icp_plane_status", k_icp_plane_status, 1, MRR_BLOCK, 0, st, (const double*)c.res,
                        c.nblk, N, (const double*)w.plane.cnt, relative_rmse_thr, max_iterations, rmse, status))
      return rc;
  }
  return MR_OK;
}

int32_t mr_icp_mesh_closest(const float* x, int64_t N, int64_t P1, const int64_t* x_lengths, const float* rts,
                            int64_t T, const int64_t* faces_first, const int64_t* faces_count, int64_t max_faces,
                            float* dist, int32_t* face, float* q, float* normal, void* ws, size_t ws_bytes,
                            void* stream) {
  if (int rc = check_icm("icp mesh closest", N, P1, T, faces_first, faces_count, max_faces)) return rc;
  if (!x || !q || !normal || !ws) return set_err(MR_EINVAL, "icp mesh closest: NULL pointer");
  const IcpMeshWS w = carve_icp_mesh(ws, N, P1, T);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "icp mesh workspace too small");
  const ICMGeom g = icm_geom(N, P1, max_faces);
  if (g.groups > 0x7fffffffll) return set_err(MR_EUNSUPPORTED, "icp mesh closest: P1 * T is too large for one launch");
  const hipStream_t st = (hipStream_t)stream;
  const IcpWS& c = w.plane.icp;
  if (int rc = memset_async(c.key, 0xff, c.key_bytes, st)) return rc;
  if (g.groups > 0)
    if (int rc = launch(KID_NONE, "k_icpm_scan", k_icpm_scan, dim3((unsigned)g.groups, (unsigned)N), ICM_BLOCK, 0, st, x,
                        P1, x_lengths, rts, (const float4*)w.rec, T, faces_first, faces_count, g,
                        (const int32_t*)nullptr, 0, c.key))
      return rc;
  return launch(KID_NONE, "k_icpm_close", k_icpm_close, dim3((unsigned)c.nblk, (unsigned)N), MRR_BLOCK, 0, st, x, P1,
                x_lengths, (const double*)nullptr, rts, (const float4*)w.rec, T, faces_first, faces_count,
                __builtin_inff(), (const int32_t*)nullptr, 0, c.key, c.idx, (float*)nullptr, (double*)nullptr, c.nblk,
                q, normal, dist, face);
}

}  // extern "C"
