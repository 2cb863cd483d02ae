// mi355r — mesh shape-prior losses (PyTorch3D mesh_edge_loss, mesh_laplacian_smoothing(method="uniform"),
// mesh_normal_consistency) for a packed batch of meshes: mr_mesh_priors_* of include/mi355r.h.
// A translation unit of its own (the render kernels of mr_raster.hip are compiled as before).
//
// The topology comes from the host, built once per faces tensor (kernels.mesh_prior_topology): unique
// edges, vertex -> neighbour CSR, the (e0, e1, a, b) list of face pairs sharing an edge, a vertex ->
// (pair, role) CSR and per-element weights 1 / (elements of that kind in the mesh * meshes).
//
//   forward  k_priors_fwd   one launch; thread i takes edge i, vertex i and pair i. Per-workgroup partial
//                           sums of the three weighted terms (double, fixed tree); for the backward the
//                           Laplacian's weighted unit vectors u_i = w_i Lv_i / |Lv_i| with 1 / deg(i)
//                           (V float4) and each pair's four weighted gradient rows (4 P float4).
//            k_priors_final one workgroup sums the partials in a fixed order into three floats.
//   backward k_priors_bwd   one launch, one vertex per thread: it GATHERS its edge and Laplacian
//                           contributions through the neighbour CSR and its pair rows through the
//                           (pair, role) CSR, scales by the three upstream scalars (read from device
//                           memory) and stores grad_verts. No atomics: bitwise reproducible.
//
// Per-element arithmetic is double (float32 in, float32 out): the Laplacian is a difference of nearly
// equal vectors on a smooth mesh and the normal term's gradient a difference of nearly equal unit
// vectors on a flat one; a few thousand elements' worth of double arithmetic costs less than a launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/mi355r.h"
#include "mr_common.h"
#include "mr_host.h"

#define MRP_BLOCK 256

namespace {

struct D3 {
  double x, y, z;
};
__device__ __forceinline__ D3 ld3(const float* __restrict__ v, int64_t i) {
  return D3{(double)v[3 * i], (double)v[3 * i + 1], (double)v[3 * i + 2]};
}
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 add(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 mul(D3 a, double s) { return D3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) {
  return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ float4 row4(D3 a, double w) {
  return make_float4((float)a.x, (float)a.y, (float)a.z, (float)w);
}

struct PriorsWS {
  double* part;  // (blocks, 3) per-workgroup partial sums
  float4* lapu;  // (V) u_i and 1 / deg(i) (0 for an isolated vertex)
  float4* prow;  // (4 P) weighted gradient of pair p's term w.r.t. its vertex of role r (e0, e1, a, b) at 4 p + r
  size_t bytes;
};
inline int64_t fwd_blocks(int64_t V, int64_t E, int64_t P) {
  const int64_t n = std::max({V, E, P});
  return n > 0 ? ceil_div(n, MRP_BLOCK) : 1;
}
PriorsWS carve_priors(void* base, int64_t V, int64_t E, int64_t P) {
  PriorsWS w;
  Carver c(base);
  w.part = c.take<double>(3 * (size_t)fwd_blocks(V, E, P));
  w.lapu = c.take<float4>((size_t)V);
  w.prow = c.take<float4>(4 * (size_t)P);
  w.bytes = c.off;
  return w;
}

__global__ void __launch_bounds__(MRP_BLOCK) k_priors_fwd(
    const float* __restrict__ verts, int64_t V, const int2* __restrict__ edges, const float* __restrict__ edge_w,
    int64_t E, const int* __restrict__ nbr_ptr, const int* __restrict__ nbr, const float2* __restrict__ vert_w,
    const int4* __restrict__ pairs, const float* __restrict__ pair_w, int64_t P, float target_length, int terms,
    double* __restrict__ part, float4* __restrict__ lapu, float4* __restrict__ prow) {
  __shared__ double sm[4];
  const int64_t i = (int64_t)blockIdx.x * MRP_BLOCK + threadIdx.x;
  double te = 0.0, tl = 0.0, tn = 0.0;

  if ((terms & MR_PRIOR_EDGE) && i < E) {
    const int2 e = edges[i];
    const D3 d = sub(ld3(verts, e.x), ld3(verts, e.y));
    const double r = sqrt(dot(d, d)) - (double)target_length;
    te = (double)edge_w[i] * (r * r);
  }

  if ((terms & MR_PRIOR_LAPLACIAN) && i < V) {
    const int b = nbr_ptr[i], n = nbr_ptr[i + 1] - b;
    D3 s{0.0, 0.0, 0.0};
    for (int k = 0; k < n; ++k) s = add(s, ld3(verts, nbr[b + k]));
    const double inv = n > 0 ? 1.0 / (double)n : 0.0;
    const D3 lv = sub(mul(s, inv), ld3(verts, i));
    const double len = sqrt(dot(lv, lv));
    const double w = (double)vert_w[i].x;
    tl = w * len;
    if (lapu) lapu[i] = row4(len > 0.0 ? mul(lv, w / len) : D3{0.0, 0.0, 0.0}, inv);
  }

  if ((terms & MR_PRIOR_NORMAL) && i < P) {
    const int4 q = pairs[i];  // e0, e1, a, b
    const D3 v0 = ld3(verts, q.x);
    const D3 d = sub(ld3(verts, q.y), v0), pa = sub(ld3(verts, q.z), v0), pb = sub(ld3(verts, q.w), v0);
    const D3 n0 = cross(d, pa), n1 = cross(pb, d);  // n1 = -(d x pb)
    const double eps = 1e-8;
    const double l0 = sqrt(dot(n0, n0)), l1 = sqrt(dot(n1, n1));
    const double m0 = l0 > eps ? l0 : eps, m1 = l1 > eps ? l1 : eps;
    const double c = dot(n0, n1) / (m0 * m1);
    const double w = (double)pair_w[i];
    tn = w * (1.0 - c);
    if (prow) {
      // d(1 - c)/dn0 = -n1 / (m0 m1) + c n0 / m0^2 (the second part only where the norm is not clamped)
      const double k = -1.0 / (m0 * m1);
      const D3 h0 = add(mul(n1, k), mul(n0, l0 >= eps ? c / (m0 * m0) : 0.0));
      const D3 h1 = add(mul(n0, k), mul(n1, l1 >= eps ? c / (m1 * m1) : 0.0));
      // n0 = d x pa, n1 = pb x d: chain to d, pa, pb
      const D3 gd = add(cross(pa, h0), cross(h1, pb));
      const D3 ga = cross(h0, d), gb = cross(d, h1);
      const D3 g0 = mul(add(add(gd, ga), gb), -1.0);
      prow[4 * i] = row4(mul(g0, w), 0.0);
      prow[4 * i + 1] = row4(mul(gd, w), 0.0);
      prow[4 * i + 2] = row4(mul(ga, w), 0.0);
      prow[4 * i + 3] = row4(mul(gb, w), 0.0);
    }
  }

  te = block_sum(te, sm);
  tl = block_sum(tl, sm);
  tn = block_sum(tn, sm);
  if (threadIdx.x == 0) {
    part[3 * (int64_t)blockIdx.x] = te;
    part[3 * (int64_t)blockIdx.x + 1] = tl;
    part[3 * (int64_t)blockIdx.x + 2] = tn;
  }
}

// out[0..2] = edge, Laplacian, normal-consistency loss: thread t sums partials t, t + 256, ... in order, then
// the fixed tree. A term left out of `terms` comes out 0 (its partials are 0).
__global__ void __launch_bounds__(MRP_BLOCK) k_priors_final(const double* __restrict__ part, int64_t nb,
                                                            float* __restrict__ out) {
  __shared__ double sm[4];
  double a = 0.0, b = 0.0, c = 0.0;
  for (int64_t i = threadIdx.x; i < nb; i += MRP_BLOCK) {
    a += part[3 * i];
    b += part[3 * i + 1];
    c += part[3 * i + 2];
  }
  a = block_sum(a, sm);
  b = block_sum(b, sm);
  c = block_sum(c, sm);
  if (threadIdx.x == 0) {
    out[0] = (float)a;
    out[1] = (float)b;
    out[2] = (float)c;
  }
}

__global__ void __launch_bounds__(MRP_BLOCK) k_priors_bwd(
    const float* __restrict__ verts, int64_t V, const int* __restrict__ nbr_ptr, const int* __restrict__ nbr,
    const float2* __restrict__ vert_w, const int* __restrict__ pair_ptr, const int* __restrict__ pair_idx,
    float target_length, const float* __restrict__ g_edge, const float* __restrict__ g_lap,
    const float* __restrict__ g_norm, const float4* __restrict__ lapu, const float4* __restrict__ prow,
    float* __restrict__ grad) {
  const int64_t i = (int64_t)blockIdx.x * MRP_BLOCK + threadIdx.x;
  if (i >= V) return;
  D3 ge{0.0, 0.0, 0.0}, gl{0.0, 0.0, 0.0}, gn{0.0, 0.0, 0.0};
  if (g_edge || g_lap) {
    const int b = nbr_ptr[i], n = nbr_ptr[i + 1] - b;
    const D3 vi = ld3(verts, i);
    for (int k = 0; k < n; ++k) {
      const int j = nbr[b + k];
      if (g_edge) {  // d/dv_i of (|v_i - v_j| - t)^2; 0 where the edge has no length
        const D3 d = sub(vi, ld3(verts, j));
        const double len = sqrt(dot(d, d));
        if (len > 0.0) ge = add(ge, mul(d, 2.0 * (len - (double)target_length) / len));
      }
      if (g_lap) {  // u_j / deg(j)
        const float4 u = lapu[j];
        gl = add(gl, mul(D3{(double)u.x, (double)u.y, (double)u.z}, (double)u.w));
      }
    }
    if (g_edge) ge = mul(ge, (double)vert_w[i].y * (double)*g_edge);
    if (g_lap) {
      const float4 u = lapu[i];
      gl = mul(sub(gl, D3{(double)u.x, (double)u.y, (double)u.z}), (double)*g_lap);
    }
  }
  if (g_norm) {
    const int b = pair_ptr[i], n = pair_ptr[i + 1] - b;
    for (int k = 0; k < n; ++k) {
      const float4 r = prow[pair_idx[b + k]];
      gn = add(gn, D3{(double)r.x, (double)r.y, (double)r.z});
    }
    gn = mul(gn, (double)*g_norm);
  }
  const D3 g = add(add(ge, gl), gn);
  grad[3 * i] = (float)g.x;
  grad[3 * i + 1] = (float)g.y;
  grad[3 * i + 2] = (float)g.z;
}

bool sizes_ok(int64_t V, int64_t E, int64_t P) {
  // element ids and CSR offsets are int32 (4 P pair rows, 2 E neighbour entries)
  return V >= 0 && E >= 0 && P >= 0 && V < 0x7fffffffll / 3 && E < 0x3fffffffll && P < 0x1fffffffll;
}

}  // namespace

extern "C" {

size_t mr_mesh_priors_workspace(int64_t V, int64_t E, int64_t P) {
  if (!sizes_ok(V, E, P)) return 0;
  return carve_priors(nullptr, V, E, P).bytes;
}

int32_t mr_mesh_priors_forward(const float* verts, int64_t V, const int32_t* edges, const float* edge_w, int64_t E,
                               const int32_t* nbr_ptr, const int32_t* nbr, const float* vert_w, const int32_t* pairs,
                               const float* pair_w, int64_t P, float target_length, int32_t terms, int32_t want_grad,
                               float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!sizes_ok(V, E, P)) return set_err(MR_EINVAL, "mesh priors: V, E or P out of range");
  if (terms & ~MR_PRIOR_ALL) return set_err(MR_EINVAL, "mesh priors: unknown bits in terms");
  if (!out || !ws) return set_err(MR_EINVAL, "mesh priors: out / workspace is NULL");
  if ((V > 0 && (!verts || !nbr_ptr || !vert_w)) || (E > 0 && (!edges || !edge_w || !nbr)) ||
      (P > 0 && (!pairs || !pair_w)))
    return set_err(MR_EINVAL, "mesh priors: NULL topology or vertex pointer");
  const PriorsWS w = carve_priors(ws, V, E, P);
  if (ws_bytes < w.bytes) return set_err(MR_EWORKSPACE, "mesh priors workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  const int64_t nb = fwd_blocks(V, E, P);
  if (int rc = launch(KID_NONE, "k_priors_fwd", k_priors_fwd, (unsigned)nb, MRP_BLOCK, 0, st, verts, V, (const int2*)edges,
                      edge_w, E, nbr_ptr, nbr, (const float2*)vert_w, (const int4*)pairs, pair_w, P, target_length, terms,
                      w.part, want_grad ? w.lapu : nullptr, want_grad ? w.prow : nullptr))
    return rc;
  return launch(KID_NONE, "k_priors_final", k_priors_final, 1, MRP_BLOCK, 0, st, w.part, nb, out);
}

int32_t mr_mesh_priors_backward(const float* verts, int64_t V, const int32_t* nbr_ptr, const int32_t* nbr,
                                const float* vert_w, const int32_t* pair_ptr, const int32_t* pair_idx, int64_t E,
                                int64_t P, float target_length, int32_t terms, const float* g_edge, const float* g_lap,
                                const float* g_norm, const void* fwd_ws, float* grad_verts, void* stream) {
  if (!sizes_ok(V, E, P)) return set_err(MR_EINVAL, "mesh priors: V, E or P out of range");
  if (terms & ~MR_PRIOR_ALL) return set_err(MR_EINVAL, "mesh priors: unknown bits in terms");
  if (V == 0) return MR_OK;
  if (!verts || !nbr_ptr || !vert_w || !pair_ptr || !fwd_ws || !grad_verts || (E > 0 && !nbr) || (P > 0 && !pair_idx))
    return set_err(MR_EINVAL, "mesh priors backward: NULL pointer");
  // a term the forward did not compute left no rows in the workspace: its upstream gradient is ignored
  if (!(terms & MR_PRIOR_EDGE)) g_edge = nullptr;
  if (!(terms & MR_PRIOR_LAPLACIAN)) g_lap = nullptr;
  if (!(terms & MR_PRIOR_NORMAL)) g_norm = nullptr;
  const PriorsWS w = carve_priors((void*)fwd_ws, V, E, P);
  return launch(KID_NONE, "k_priors_bwd", k_priors_bwd, ceil_div(V, MRP_BLOCK), MRP_BLOCK, 0, (hipStream_t)stream, verts, V,
                nbr_ptr, nbr, (const float2*)vert_w, pair_ptr, pair_idx, target_length, g_edge, g_lap, g_norm, w.lapu, w.prow,
                grad_verts);
}

}  // extern "C"
