// mi355r — point-to-triangle distances (PyTorch3D point_mesh_face_distance / point_face_distance /
// face_point_distance): mr_point_face_nearest / mr_point_mesh_face_* of include/mi355r.h. A translation unit of
// its own, over mr_host.h and mr_common.h like the others.
//
//   mr_tri.h        the pair function (tri_make / seg_dist / pair_dist), the triangle record and its staged form, and
//                   the compare loop of a staged chunk, shared with mr_icpmesh.hip.
//   k_pm_nn         both directions of a packed batch in one launch, grid (groups, mesh, direction), shaped like
//                   k_nn of mr_points.hip. point -> face: a thread keeps 2 points in registers, the workgroup stages a
//                   chunk of <= 256 triangle records (7 float4 each, 28 KiB) in LDS; every lane reads the same record
//                   (a broadcast) and the record's plane flag is wave-uniform, so a triangle below the area threshold
//                   costs the three segment terms only. face -> point: a thread keeps one triangle record in
//                   registers, the chunk holds <= 1024 points as float4. Chunks merge with a 64-bit atomicMin on
//                   nn_key (mr_cloud.h) of the distance and the index within the mesh; the in-chunk comparison is
//                   strict, so equal distances resolve to the lowest index.
//   k_pm_reduce     keys -> dist / idx per point and per face (0 / -1 without a counterpart), float64 partial sums.
//   k_pm_final      per mesh: partial sums in order, 1/P_n and 1/T_n, then the batch in a fixed tree and 1/N; leaves
//                   the backward's coefficients.
//   k_pm_bwd        one launch over points and faces: every winner recomputes its pair's closest point with
//                   pair_dist; a point's own row is a store, everything many-to-one goes through fix_add.
//   k_pm_fix_out    own rows + fixed-point rows -> float32, once. (The backward's one memset covers a multiple of
//                   256 B: no separate clear of grad_points, whose 12 P bytes need not be a multiple of 8.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mi355r.h"
#include "mr_common.h"
#include "mr_host.h"
#include "mr_cloud.h"
#include "mr_tri.h"

#define MPM_BLOCK 256                    // threads of every kernel here (four waves)
#define MPM_Q 2                          // points per thread, point -> face
#define MPM_PTILE (MPM_BLOCK * MPM_Q)    // points per workgroup, point -> face
#define MPM_FTILE MPM_BLOCK              // faces per workgroup, face -> point (one per thread)
#define MPM_TRI_MAXCHUNK 256             // triangles staged per workgroup at most (28 KiB of LDS)
#define MPM_TRI_MINCHUNK 32
#define MPM_PT_MAXCHUNK 1024             // points staged per workgroup at most (16 KiB)
#define MPM_PT_MINCHUNK 64
#define MPM_WANT_GROUPS 1024             // workgroups per direction the chunk size aims for
#define MPM_PER 4                        // elements per thread of k_pm_reduce
#define MPM_RTILE (MPM_BLOCK * MPM_PER)

namespace {

// The packed batch: points (P,3), verts (V,3), faces (T,3) over packed vertex ids; per mesh the first element and
// the count of its points and of its faces (device arrays, never read by the host).
struct PMBatch {
  const float* pts;
  const float* verts;
  const int32_t* faces;
  const int64_t *pf, *pc, *ff, *fc;
  int64_t P, V, T, N;
  float min_area;
};

struct PMGeom {
  int tile[2];        // queries per workgroup of direction d (d = 0: queries points, targets faces)
  int chunk[2];       // targets per workgroup
  int64_t nchunk[2];  // chunks
  int64_t groups[2];  // workgroups per mesh
};

PMGeom pm_geom(int64_t N, int64_t max_points, int64_t max_faces) {
  PMGeom g;
  for (int d = 0; d < 2; ++d) {
    const int64_t Pq = d ? max_faces : max_points, Pt = d ? max_points : max_faces;
    const int lo = d ? MPM_PT_MINCHUNK : MPM_TRI_MINCHUNK, hi = d ? MPM_PT_MAXCHUNK : MPM_TRI_MAXCHUNK;
    g.tile[d] = d ? MPM_FTILE : MPM_PTILE;
    const int64_t qtiles = (Pq + g.tile[d] - 1) / g.tile[d];
    int64_t want = MPM_WANT_GROUPS / (N * (qtiles > 1 ? qtiles : 1));
    if (want < 1) want = 1;
    int64_t c = ((Pt + want - 1) / want + lo - 1) / lo * lo;
    if (c < lo) c = lo;
    if (c > hi) c = hi;
    g.chunk[d] = (int)c;
    g.nchunk[d] = (Pt + c - 1) / c;
    g.groups[d] = qtiles * g.nchunk[d];
  }
  return g;
}

MR_DEV Tri tri_load(const PMBatch& b, int64_t f, int& ia, int& ib, int& ic) {
  return tri_load(b.verts, b.V, b.faces, b.min_area, f, ia, ib, ic);
}

__global__ void __launch_bounds__(MPM_BLOCK) k_pm_nn(PMBatch b, PMGeom g, u64* __restrict__ key_p,
                                                     u64* __restrict__ key_f) {
  __shared__ float4 sm[MPM_TRI_MAXCHUNK * MPM_REC];  // triangle records, or MPM_PT_MAXCHUNK points
  const int d = blockIdx.z;
  if ((int64_t)blockIdx.x >= g.groups[d]) return;
  const int64_t n = blockIdx.y;
  int64_t fp, lp, ff, lf;
  range_of(b.pf, b.pc, n, b.P, fp, lp);
  range_of(b.ff, b.fc, n, b.T, ff, lf);
  const int64_t lq = d ? lf : lp, lt = d ? lp : lf;
  const int64_t q0 = ((int64_t)blockIdx.x / g.nchunk[d]) * g.tile[d];
  const int64_t t0 = ((int64_t)blockIdx.x % g.nchunk[d]) * g.chunk[d];
  if (q0 >= lq || t0 >= lt) return;  // uniform over the workgroup
  const int cnt = (int)((lt - t0 < g.chunk[d]) ? lt - t0 : g.chunk[d]);
  int ia, ib, ic;

  if (d == 0) {
    for (int j = threadIdx.x; j < cnt; j += MPM_BLOCK) tri_stage(sm + MPM_REC * j, tri_load(b, ff + t0 + j, ia, ib, ic));
    __syncthreads();
    float p[MPM_Q][3], best[MPM_Q];
    int bi[MPM_Q];
#pragma unroll
    for (int k = 0; k < MPM_Q; ++k) {
      const int64_t i = q0 + k * MPM_BLOCK + threadIdx.x;
      const bool ok = i < lq;
#pragma unroll
      for (int c = 0; c < 3; ++c) p[k][c] = ok ? b.pts[3 * (fp + i) + c] : 0.0f;
      best[k] = __builtin_inff();
      bi[k] = -1;
    }
    tri_scan<MPM_Q>(sm, cnt, p, best, bi);
#pragma unroll
    for (int k = 0; k < MPM_Q; ++k) {
      const int64_t i = q0 + k * MPM_BLOCK + threadIdx.x;
      if (i < lq && bi[k] >= 0)
        atomicMin(&key_p[fp + i], nn_key(best[k], (uint32_t)(t0 + bi[k])));
    }
  } else {
    for (int j = threadIdx.x; j < cnt; j += MPM_BLOCK) {
      const float* q = b.pts + 3 * (fp + t0 + j);
      sm[j] = make_float4(q[0], q[1], q[2], 0.0f);
    }
    __syncthreads();
    const int64_t i = q0 + threadIdx.x;
    if (i >= lq) return;
    const Tri t = tri_load(b, ff + i, ia, ib, ic);
    if (t.plane < 0) return;
    float best = __builtin_inff();
    int bi = -1;
#pragma unroll 2
    for (int j = 0; j < cnt; ++j) {
      const float4 q = sm[j];
      const float p[3] = {q.x, q.y, q.z};
      const float dd = pair_dist<false>(p, t, nullptr);
      if (dd < best) {
        best = dd;
        bi = j;
      }
    }
    if (bi >= 0) atomicMin(&key_f[ff + i], nn_key(best, (uint32_t)(t0 + bi)));
  }
}

// grid (nblk, N, 2). dist / idx / part may each be NULL. A key no scan wrote (no counterpart, or a face that is
// not a triangle of the mesh) gives 0 / -1.
__global__ void __launch_bounds__(MPM_BLOCK) k_pm_reduce(PMBatch b, const u64* __restrict__ key_p,
                                                         const u64* __restrict__ key_f, float* __restrict__ dist_p,
                                                         int32_t* __restrict__ idx_p, float* __restrict__ dist_f,
                                                         int32_t* __restrict__ idx_f, double* __restrict__ part,
                                                         int64_t nblk) {
  __shared__ double sm[4];
  const int d = blockIdx.z;
  const int64_t n = blockIdx.y;
  int64_t fq, lq;
  range_of(d ? b.ff : b.pf, d ? b.fc : b.pc, n, d ? b.T : b.P, fq, lq);
  const u64* __restrict__ key = d ? key_f : key_p;
  float* __restrict__ dist = d ? dist_f : dist_p;
  int32_t* __restrict__ idx = d ? idx_f : idx_p;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < MPM_PER; ++k) {
    const int64_t i = (int64_t)blockIdx.x * MPM_RTILE + k * MPM_BLOCK + threadIdx.x;
    if (i >= lq) continue;
    const u64 kk = key[fq + i];
    const bool ok = kk != ~0ull;
    const float dv = ok ? key_dist(kk) : 0.0f;
    if (dist) dist[fq + i] = dv;
    if (idx) idx[fq + i] = ok ? (int32_t)key_index(kk) : -1;
    s += (double)dv;
  }
  if (part) {  // uniform
    s = block_sum(s, sm);
    if (threadIdx.x == 0) part[((int64_t)d * b.N + n) * nblk + blockIdx.x] = s;
  }
}

// One workgroup. Thread t takes meshes t, t + 256, ...: each mesh's partials are summed in order, divided by its
// point and face counts; the meshes' values are summed per thread in order, then in the fixed tree, then / N.
// coef (2, N): d loss / d (one distance of direction d of mesh n) for an upstream gradient of 1; 0 for a pair whose
// cloud or mesh is empty.
__global__ void __launch_bounds__(MPM_BLOCK) k_pm_final(PMBatch b, const double* __restrict__ part, int64_t nblk,
                                                        float* __restrict__ out, float* __restrict__ coef) {
  __shared__ double sm[4];
  const double inv_n = 1.0 / (double)b.N;
  double total = 0.0;
  for (int64_t n = threadIdx.x; n < b.N; n += MPM_BLOCK) {
    int64_t f, lp, lf;
    range_of(b.pf, b.pc, n, b.P, f, lp);
    range_of(b.ff, b.fc, n, b.T, f, lf);
    const bool both = lp > 0 && lf > 0;
    for (int d = 0; d < 2; ++d) {
      const double c = both ? 1.0 / (double)(d ? lf : lp) : 0.0;
      double s = 0.0;
      for (int64_t k = 0; k < nblk; ++k) s += part[((int64_t)d * b.N + n) * nblk + k];
      total += c * s;
      if (coef) coef[(int64_t)d * b.N + n] = (float)(c * inv_n);
    }
  }
  total = block_sum(total, sm);
  if (threadIdx.x == 0) out[0] = (float)(total * inv_n);
}

// grid (blocks over max(points, faces) of a mesh, N, 2). Direction 0: point i stores its own gradient row and adds
// the three vertex rows; direction 1: face i adds its nearest point's row and its own three vertex rows. The weight
// of a distance is wp[point] / wf[face] where given, else coef[d, n] * up[0]. fix / rem: rows of the points (3 P)
// then of the vertices (3 V); own (3 P): the points' own rows, cleared with them.
__global__ void __launch_bounds__(MPM_BLOCK) k_pm_bwd(PMBatch b, const int32_t* __restrict__ idx_p,
                                                      const int32_t* __restrict__ idx_f, const float* __restrict__ coef,
                                                      const float* __restrict__ up, const float* __restrict__ wp,
                                                      const float* __restrict__ wf, float* __restrict__ own,
                                                      u64* __restrict__ fix, float* __restrict__ rem) {
  const int d = blockIdx.z;
  const int64_t n = blockIdx.y;
  int64_t fp, lp, ff, lf;
  range_of(b.pf, b.pc, n, b.P, fp, lp);
  range_of(b.ff, b.fc, n, b.T, ff, lf);
  const int64_t i = (int64_t)blockIdx.x * MPM_BLOCK + threadIdx.x;
  if (i >= (d ? lf : lp)) return;
  const int32_t* __restrict__ idx = d ? idx_f : idx_p;
  const int64_t self = (d ? ff : fp) + i;
  const int32_t j = idx ? idx[self] : -1;
  const bool has = j >= 0 && j < (d ? lp : lf);
  float g[3] = {0.0f, 0.0f, 0.0f};
  if (has) {
    const int64_t pi = d ? fp + j : self, fi = d ? self : ff + j;
    const float* per = d ? wf : wp;
    const float w = per ? per[self] : coef[(int64_t)d * b.N + n] * up[0];
    int iv[3];
    const Tri t = tri_load(b, fi, iv[0], iv[1], iv[2]);
    if (t.plane >= 0) {
      const float p[3] = {b.pts[3 * pi], b.pts[3 * pi + 1], b.pts[3 * pi + 2]};
      float bw[3];
      pair_dist<true>(p, t, bw);
      const float w2 = 2.0f * w;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float c = (bw[0] * t.v0[k] + bw[1] * t.v1[k]) + bw[2] * t.v2[k];  // the closest point
        g[k] = w2 * (p[k] - c);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) fix_add(fix, rem, 3 * (b.P + (int64_t)iv[c]) + k, -(bw[c] * g[k]));
      if (d) {
#pragma unroll
        for (int k = 0; k < 3; ++k) fix_add(fix, rem, 3 * pi + k, g[k]);
      }
    }
  }
  if (!d && has) {
#pragma unroll
    for (int k = 0; k < 3; ++k) own[3 * self + k] = g[k];
  }
}

// grad_points = the points' own rows + their many-to-one rows; grad_verts = the vertices' rows.
__global__ void __launch_bounds__(MPM_BLOCK) k_pm_fix_out(const u64* __restrict__ fix, const float* __restrict__ rem,
                                                          const float* __restrict__ own, int64_t np, int64_t nv,
                                                          float* __restrict__ grad_points,
                                                          float* __restrict__ grad_verts) {
  const int64_t i = (int64_t)blockIdx.x * MPM_BLOCK + threadIdx.x;
  if (i < np) grad_points[i] = own[i] + fix_read(fix, rem, i);
  else if (i < np + nv) grad_verts[i - np] = fix_read(fix, rem, i);
}

struct PMWS {
  u64* key[2];   // (P), (T)
  double* part;  // (2, N, nblk)
  int64_t nblk;
  size_t key_bytes, bytes;
};
PMWS carve_pm(void* base, int64_t N, int64_t P, int64_t T) {
  PMWS w;
  Carver c(base);
  w.key[0] = c.take_packed<u64>((size_t)P);  // the two key arrays back to back: one memset
  w.key[1] = c.take<u64>((size_t)T);
  w.key_bytes = sizeof(u64) * (size_t)(P + T);
  w.nblk = ceil_div(P > T ? P : T, MPM_RTILE);
  if (w.nblk < 1) w.nblk = 1;
  w.part = c.take<double>(2 * (size_t)(N * w.nblk));
  w.bytes = c.off;
  return w;
}

struct PMBwdWS {
  u64* fix;
  float* rem;
  float* own;
  size_t bytes;
};
PMBwdWS carve_pm_bwd(void* base, int64_t P, int64_t V) {
  PMBwdWS w;
  Carver c(base);
  const size_t n = 3 * (size_t)(P + V);
  w.fix = c.take_packed<u64>(n);  // words, remainders and own rows back to back: one memset of a 256-B multiple
  w.rem = c.take_packed<float>(n);
  w.own = c.take<float>(3 * (size_t)P);
  w.bytes = c.off;
  return w;
}

bool pm_sizes_ok(int64_t N, int64_t P, int64_t T, int64_t V) {
  // indices within a mesh are int32; the grid's y dimension is the batch
  const int64_t lim = 0x7fffffffll / 3;
  return N >= 1 && N <= 65535 && P >= 0 && T >= 0 && V >= 0 && P < lim && T < lim && V < lim;
}

int check_pm(const char* who, const float* points, int64_t P, const int64_t* pf, const int64_t* pc, int64_t max_points,
             const float* verts, int64_t V, const int32_t* faces, int64_t T, const int64_t* ff, const int64_t* fc,
             int64_t max_faces, int64_t N, float min_area) {
  if (N < 1) return set_err(MR_EINVAL, "%s: N must be >= 1", who);
  if (P < 0 || T < 0 || V < 0) return set_err(MR_EINVAL, "%s: P, T and V must be >= 0", who);
  if (!pm_sizes_ok(N, P, T, V))
    return set_err(MR_EUNSUPPORTED, "%s: more than 65535 meshes or a batch too large for 32-bit indices", who);
  if (max_points < 0 || max_points > P || max_faces < 0 || max_faces > T)
    return set_err(MR_EINVAL, "%s: max_points / max_faces outside [0, P] / [0, T]", who);
  if (!(min_area >= 0.0f)) return set_err(MR_EINVAL, "%s: min_triangle_area must be >= 0", who);
  if (!pf || !pc || !ff || !fc) return set_err(MR_EINVAL, "%s: a first / count array is NULL", who);
  if ((P > 0 && !points) || (T > 0 && (!faces || !verts)))
    return set_err(MR_EINVAL, "%s: points / verts / faces is NULL", who);
  return MR_OK;
}

PMBatch pm_batch(const float* points, int64_t P, const int64_t* pf, const int64_t* pc, const float* verts, int64_t V,
                 const int32_t* faces, int64_t T, const int64_t* ff, const int64_t* fc, int64_t N, float min_area) {
  PMBatch b;
  b.pts = points;
  b.verts = verts;
  b.faces = faces;
  b.pf = pf;
  b.pc = pc;
  b.ff = ff;
  b.fc = fc;
  b.P = P;
  b.V = V;
  b.T = T;
  b.N = N;
  b.min_area = min_area;
  return b;
}

// memset of the keys, k_pm_nn, k_pm_reduce. Returns the number of partial sums per (direction, mesh) in nblk.
int run_pm(const PMBatch& b, int64_t max_points, int64_t max_faces, const PMWS& w, float* dist_p, int32_t* idx_p,
           float* dist_f, int32_t* idx_f, double* part, int64_t& nblk, hipStream_t st) {
  const PMGeom g = pm_geom(b.N, max_points, max_faces);
  if (g.groups[0] > 0x7fffffffll || g.groups[1] > 0x7fffffffll)
    return set_err(MR_EUNSUPPORTED, "point-face nearest: points * faces is too large for one launch");
  if (w.key_bytes)
    if (int rc = memset_async(w.key[0], 0xff, w.key_bytes, st)) return rc;
  const int64_t gx = g.groups[1] > g.groups[0] ? g.groups[1] : g.groups[0];
  if (gx > 0)
    if (int rc = launch(KID_NONE, "k_pm_nn", k_pm_nn, dim3((unsigned)gx, (unsigned)b.N, 2), MPM_BLOCK, 0, st, b, g, w.key[0],
                        w.key[1]))
      return rc;
  nblk = ceil_div(max_points > max_faces ? max_points : max_faces, MPM_RTILE);
  if (nblk < 1) nblk = 1;
  return launch(KID_NONE, "k_pm_reduce", k_pm_reduce, dim3((unsigned)nblk, (unsigned)b.N, 2), MPM_BLOCK, 0, st, b,
                (const u64*)w.key[0], (const u64*)w.key[1], dist_p, idx_p, dist_f, idx_f, part, nblk);
}

}  // namespace

extern "C" {

size_t mr_point_face_nearest_workspace(int64_t N, int64_t P, int64_t T) {
  if (!pm_sizes_ok(N, P, T, 0)) return 0;
  return carve_pm(nullptr, N, P, T).bytes;
}

int32_t mr_point_face_nearest(const float* points, int64_t P, const int64_t* points_first, const int64_t* points_count,
                              int64_t max_points, const float* verts, int64_t V, const int32_t* faces, int64_t T,
                              const int64_t* faces_first, const int64_t* faces_count, int64_t max_faces, int64_t N,
                              float min_triangle_area, float* dist_p, int32_t* idx_p, float* dist_f, int32_t* idx_f,
                              void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_pm("point-face nearest", points, P, points_first, points_count, max_points, verts, V, faces, T,
                        faces_first, faces_count, max_faces, N, min_triangle_area))
    return rc;
  if (!ws) return set_err(MR_EINVAL, "point-face nearest: the workspace is NULL");
  const PMWS w = carve_pm(ws, N, P, T);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "point-face nearest workspace too small");
  const PMBatch b = pm_batch(points, P, points_first, points_count, verts, V, faces, T, faces_first, faces_count, N,
                             min_triangle_area);
  int64_t nblk;
  return run_pm(b, max_points, max_faces, w, dist_p, idx_p, dist_f, idx_f, nullptr, nblk, (hipStream_t)stream);
}

size_t mr_point_mesh_face_workspace(int64_t N, int64_t P, int64_t T) { return mr_point_face_nearest_workspace(N, P, T); }

int32_t mr_point_mesh_face_forward(const float* points, int64_t P, const int64_t* points_first,
                                   const int64_t* points_count, int64_t max_points, const float* verts, int64_t V,
                                   const int32_t* faces, int64_t T, const int64_t* faces_first,
                                   const int64_t* faces_count, int64_t max_faces, int64_t N, float min_triangle_area,
                                   int32_t* idx_p, int32_t* idx_f, float* coef, float* out, void* ws, size_t ws_bytes,
                                   void* stream) {
  if (int rc = check_pm("point-mesh face distance", points, P, points_first, points_count, max_points, verts, V, faces,
                        T, faces_first, faces_count, max_faces, N, min_triangle_area))
    return rc;
  if (!out || !ws) return set_err(MR_EINVAL, "point-mesh face distance: out / workspace is NULL");
  const PMWS w = carve_pm(ws, N, P, T);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "point-mesh face distance workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  const PMBatch b = pm_batch(points, P, points_first, points_count, verts, V, faces, T, faces_first, faces_count, N,
                             min_triangle_area);
  int64_t nblk;
  if (int rc = run_pm(b, max_points, max_faces, w, nullptr, idx_p, nullptr, idx_f, w.part, nblk, st)) return rc;
  return launch(KID_NONE, "k_pm_final", k_pm_final, 1, MPM_BLOCK, 0, st, b, (const double*)w.part, nblk, out, coef);
}

size_t mr_point_mesh_face_backward_workspace(int64_t P, int64_t V) {
  if (!pm_sizes_ok(1, P, 0, V)) return 0;
  return carve_pm_bwd(nullptr, P, V).bytes;
}

int32_t mr_point_mesh_face_backward(const float* points, int64_t P, const int64_t* points_first,
                                    const int64_t* points_count, int64_t max_points, const float* verts, int64_t V,
                                    const int32_t* faces, int64_t T, const int64_t* faces_first,
                                    const int64_t* faces_count, int64_t max_faces, int64_t N, float min_triangle_area,
                                    const int32_t* idx_p, const int32_t* idx_f, const float* coef, const float* grad_out,
                                    const float* grad_dist_p, const float* grad_dist_f, float* grad_points,
                                    float* grad_verts, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_pm("point-mesh face backward", points, P, points_first, points_count, max_points, verts, V, faces,
                        T, faces_first, faces_count, max_faces, N, min_triangle_area))
    return rc;
  if ((idx_p && !grad_dist_p && (!coef || !grad_out)) || (idx_f && !grad_dist_f && (!coef || !grad_out)))
    return set_err(MR_EINVAL, "point-mesh face backward: a direction has neither coef and grad_out nor its grad_dist");
  if ((P > 0 && !grad_points) || (V > 0 && !grad_verts) || !ws)
    return set_err(MR_EINVAL, "point-mesh face backward: grad_points / grad_verts / workspace is NULL");
  const PMBwdWS w = carve_pm_bwd(ws, P, V);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "point-mesh face backward workspace too small");
  if (P + V == 0) return MR_OK;
  const hipStream_t st = (hipStream_t)stream;
  const PMBatch b = pm_batch(points, P, points_first, points_count, verts, V, faces, T, faces_first, faces_count, N,
                             min_triangle_area);
  if (int rc = memset_async(ws, 0, w.bytes, st)) return rc;
  const int64_t mx = max_points > max_faces ? max_points : max_faces;
  if (mx > 0)
    if (int rc = launch(KID_NONE, "k_pm_bwd", k_pm_bwd, dim3((unsigned)ceil_div(mx, MPM_BLOCK), (unsigned)N, 2), MPM_BLOCK, 0,
                        st, b, idx_p, idx_f, coef, grad_out, grad_dist_p, grad_dist_f, w.own, w.fix, w.rem))
      return rc;
  return launch(KID_NONE, "k_pm_fix_out", k_pm_fix_out, (unsigned)ceil_div(3 * (P + V), MPM_BLOCK), MPM_BLOCK, 0, st,
                (const u64*)w.fix, (const float*)w.rem, (const float*)w.own, 3 * P, 3 * V, grad_points, grad_verts);
}

}  // extern "C"
