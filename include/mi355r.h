/*
 * mi355r — MI355X-native differentiable mesh rasterizer: public C ABI.
 *
 * Plain pointers + sizes, no torch types. All device pointers live in HBM of
 * the current HIP device; every call is asynchronous on `stream` (a
 * hipStream_t passed as void*) and performs no host synchronisation and no
 * device allocation: callers own outputs and workspace (sized with the
 * *_workspace() queries). Returns MR_OK (0) or an error code; the message is
 * in mr_last_error() (thread-local).
 *
 * Boundary being replaced (reference path: torch_renderer.py:97-159,
 * renderer.py:87-101 -> PyTorch3D MeshRasterizer/MeshRenderer ->
 * pybind11 module pytorch3d._C, upstream csrc/ext.cpp):
 *   _C.rasterize_meshes           -> mr_rasterize_meshes
 *   _C.rasterize_meshes_backward  -> mr_rasterize_meshes_backward
 *   MeshRasterizer.transform (torch bmm) -> mr_project_faces(+_backward)
 *   SoftPhongShader + SoftSilhouetteShader + zbuf relu over ONE raster pass
 *     (torch_renderer.py:110-121 rasterizes twice; :155-159 once more)
 *                                -> mr_render_forward / mr_render_backward
 */
#ifndef MI355R_H
#define MI355R_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MR_OK = 0, MR_EINVAL = 1, MR_ELAUNCH = 2, MR_EUNSUPPORTED = 3, MR_EWORKSPACE = 4 };

/* Per-view camera: X_view = X_world @ R + T (PyTorch3D row-vector
 * convention, R row-major), ndc = (ax * x/z + bx, ay * y/z + by, z).
 * PerspectiveCameras(in_ndc=False): ax = fx/s, bx = (W/2 - px)/s, s = min(H,W)/2
 * (torch_renderer.py:61-71); FoVPerspectiveCameras: ax = 1/(tan(fov/2)*aspect).
 * 64 bytes. */
typedef struct mr_view {
  float R[9];
  float T[3];
  float ax, bx, ay, by;
} mr_view_t;

/* RasterizationSettings (upstream rasterizer.py) — blur/K/clip/cull as there. */
typedef struct mr_raster_settings {
  int32_t H, W;
  int32_t faces_per_pixel;   /* 1..128 on mr_rasterize_meshes; 1 on the fused mr_render_* path */
  float blur_radius;
  int32_t perspective_correct;
  int32_t clip_barycentric_coords;
  int32_t cull_backfaces;
  int32_t max_faces_per_bin; /* <= 0: library default; overflow is handled exactly */
  /* Near-plane clipping (upstream MeshRasterizer: z_clip_value = znear / 2 for FoVPerspectiveCameras,
   * then mesh/clip.py clip_faces -> rasterize -> convert_clipped_rasterization_to_original_faces).
   * clip_z != 0: faces crossing view z = z_clip_value are split (one or two sub-triangles, the two
   * halves of a clipped quadrilateral being each other's clipped_faces_neighbor_idx); outputs refer
   * to the original faces (pix_to_face, barycentrics converted back); backward chains through the
   * split. Done inside the binning kernels: no host round trip, nothing to do when nothing crosses. */
  int32_t clip_z;
  float z_clip_value;
} mr_raster_settings_t;

/* Shading / blending parameters (SoftPhongShader, PointLights, Materials,
 * BlendParams, SoftSilhouetteShader). */
typedef struct mr_shade_params {
  int32_t light_kind;        /* 0 = PointLights, 1 = AmbientLights */
  float light_location[3];
  float light_ambient[3], light_diffuse[3], light_specular[3];
  float mat_ambient[3], mat_diffuse[3], mat_specular[3];
  float shininess;
  float sigma_rgb, gamma, background[3], znear, zfar;
  float sigma_sil;
  int32_t out_flags;         /* MR_OUT_* */
  int32_t rgb_channels;      /* 3 (rgb) or 4 (rgba, alpha = 1 - prod(1 - prob)) */
} mr_shade_params_t;

enum { MR_OUT_DEPTH = 1, MR_OUT_SIL = 2, MR_OUT_RGB = 4,
       /* with MR_OUT_RGB, mr_shade_fragments_* only: upstream hard_rgb_blend (HardPhongShader) —
        * the nearest fragment's Phong colour or the background, alpha = 1 where a face covers the
        * pixel; gradients reach the colour of the nearest fragment only */
       MR_OUT_HARD = 8,
       /* mr_render_backward[_opencv] only: the forward workspace's per-face gradient totals are as the
        * forward left them (cleared), i.e. this is the first backward over that forward; the
        * backward then skips clearing them. Leave it unset for any later backward over the same
        * forward workspace (e.g. autograd retain_graph). */
       MR_GRAD_ROWS_CLEARED = 16,
       /* with MR_OUT_SIL, mr_render_forward/_backward[_opencv]: the silhouette buffer is (N,H,W,4)
        * RGBA as SoftSilhouetteShader returns it, (1, 1, 1, alpha) per pixel, written by the
        * kernels; its gradient is the (N,H,W,4) gradient of that tensor (channel 3 is read) */
       MR_OUT_SIL_RGBA = 32,
       /* with MR_OUT_DEPTH, mr_render_forward/_backward[_opencv]: the depth buffer is MeshRasterizer's
        * zbuf[..., 0] of K = 1 fragments (the nearest face's depth, -1 where no face) instead of
        * DepthRender's relu of it (camera_pose_optimizer.py:244-246 reads rasterizer(...).zbuf). */
       MR_OUT_ZBUF = 64,
       /* bits 8-9 (MR_SREC_SLOT(k), k < 4), mr_render_forward / _reshade / _backward: which of the forward
        * workspace's four per-face shading-record sets this call packs and its backward reads (0 for a
        * plain forward; mr_render_reshade calls sharing one workspace take distinct slots) */
       MR_SREC_SLOT_SHIFT = 8,
       /* mr_shade_fragments_* only: every pixel's empty slots (pix_to_face = -1) follow its filled
        * ones, as mr_rasterize_meshes[_world] (and PyTorch3D's rasterizer) write them; the kernels
        * then stop at a pixel's first empty slot instead of reading all K (same results).
        * Bit 10 since mr_version() 5 (it was 64, the value of MR_OUT_ZBUF, before). */
       MR_FRAG_SORTED = 1024 };

/* One triangle mesh shared by all N views (Meshes.extend(N)) — or, with
 * view_face_first set, a batch of N distinct meshes (renderer.py:78-80: N OBJ files in one Meshes),
 * view n rendering mesh n: the arrays then hold the meshes' union (each mesh's faces index its own
 * vertices inside the union; no vertex is shared between meshes). */
typedef struct mr_mesh {
  const float* verts;        /* (V,3) world */
  int64_t V;
  const int32_t* faces;      /* (F,3) */
  int64_t F;
  const int32_t* vadj_ptr;   /* (V+1) CSR vertex -> (face<<2 | corner), sorted by (corner, face) */
  const int32_t* vadj;
  const float* vnormals;     /* (V,3) from mr_vertex_normals (PointLights only) */
  int32_t tex_kind;          /* 0 white, 1 per-vertex colours, 2 UV map */
  const float* vcolors;      /* (V,3) */
  const float* verts_uvs;    /* (Vt,2) */
  const int32_t* faces_uvs;  /* (F,3) */
  const float* tex_rgba;     /* (Ht,Wt,4) float, image row 0 first (flip done in-kernel) */
  int32_t tex_h, tex_w;
  /* Optional (mr_render_forward only): when non-NULL the forward computes the vertex normals
   * itself into vnormals_out (V,3) and their un-normalised sums into vraw_out (V,3), in its first
   * launch, instead of reading `vnormals` (saves the separate mr_vertex_normals launch). */
  float* vnormals_out;
  float* vraw_out;
  /* Optional: the same map as 8-bit texels, (Ht,Wt,4) u8, when every value of tex_rgba is exactly
   * tex_lut[k] for some k (e.g. a PNG divided by 255): the samplers then read 4-B texels and
   * convert through the 256-entry table, bitwise the same values at a quarter of the bytes. */
  const uint8_t* tex_u8;
  const float* tex_lut;      /* (256) f32, required with tex_u8 */
  /* Distinct meshes (mr_render_*, mr_shade_fragments_*; NULL: one shared mesh). Device arrays:
   * view_face_first (N+1) the first union face of view n's mesh (view_face_first[N] = F) and
   * view_face_count (N) its face count; max_view_faces (host) = the largest count. Face ids stay
   * union face ids (= PyTorch3D's packed ids of the batch). Size the forward workspace with
   * mr_render_workspace_meshes. */
  const int64_t* view_face_first;
  const int64_t* view_face_count;
  int64_t max_view_faces;
} mr_mesh_t;

const char* mr_last_error(void);
int32_t mr_version(void);
/* sizeof of the ABI structs as compiled into the library (binding self-check):
 * 0 mr_view_t, 1 mr_raster_settings_t, 2 mr_shade_params_t, 3 mr_mesh_t; -1 otherwise. */
int32_t mr_struct_size(int32_t which);
/* Host only (no GPU): the pixels p0 .. p1 along an image axis of S1 pixels (S2 = the other side) whose centres
 * can lie inside the NDC interval [lo, hi] — the rule behind the binning's tile rectangles and the rasters'
 * candidate rectangles, run on the CPU from the kernels' own source. Pass the padded interval (bbox -/+
 * sqrt(blur_radius)). The range is before any clip to a tile; p0 > p1 means no pixel. */
int32_t mr_pixel_range(float lo, float hi, int32_t S1, int32_t S2, int32_t* p0, int32_t* p1);

/* ---------------- PyTorch3D _C.rasterize_meshes boundary ---------------- */
size_t mr_rasterize_meshes_workspace(int64_t num_meshes, int64_t total_faces, int32_t H, int32_t W,
                                     int32_t max_faces_per_bin);

/* face_verts (F,3,3) NDC xy + view z; mesh_to_face_first_idx / num_faces_per_mesh (N) int64 on device.
 * Outputs (N,H,W,K): pix_to_face int64 (packed face id or -1), zbuf, dists f32; bary (N,H,W,K,3). */
int32_t mr_rasterize_meshes(const float* face_verts, const int64_t* mesh_to_face_first_idx,
                            const int64_t* num_faces_per_mesh, int64_t num_meshes, int64_t total_faces,
                            const mr_raster_settings_t* settings, int64_t* pix_to_face, float* zbuf,
                            float* bary, float* dists, void* workspace, size_t workspace_bytes, void* stream);

/* Camera poses in the PyTorch3D convention (row-vector R (N,3,3), T (N,3); X_view = X_world R + T) with
 * the intrinsics rows {ax, bx, ay, by} (N,4) of mr_view_t; *_stride = floats between consecutive views
 * (0 broadcasts one row). Same layout as mr_opencv_poses_t. */
typedef struct mr_poses {
  const float* R;
  int64_t R_stride;
  const float* T;
  int64_t T_stride;
  const float* intr;
  int64_t intr_stride;
} mr_poses_t;

/* MeshRasterizer.forward for ONE mesh shared by N views (Meshes.extend; upstream
 * mesh/rasterizer.py transform + rasterize_meshes): verts (V,3) f32, faces (F,3) i32. Writes the
 * fragments (as mr_rasterize_meshes, packed face ids n*F + f), face_verts (N*F,3,3) — what
 * _RasterizeFaceVerts saves for mr_rasterize_meshes_backward, bitwise mr_project_faces' output — and
 * the view records views_out (N) for mr_project_faces_backward. The projection runs inside the
 * binning's first launch (no separate projection launch, no counter memset). */
size_t mr_rasterize_meshes_world_workspace(int64_t N, int64_t F, int32_t H, int32_t W, int32_t max_faces_per_bin);
int32_t mr_rasterize_meshes_world(const float* verts, int64_t V, const int32_t* faces, int64_t F,
                                  const mr_poses_t* poses, int64_t N, const mr_raster_settings_t* settings,
                                  mr_view_t* views_out, float* face_verts, int64_t* pix_to_face, float* zbuf,
                                  float* bary, float* dists, void* workspace, size_t workspace_bytes, void* stream);

/* Measurement helper (bench.py's per-kernel algorithmic bytes): output pixels whose background the
 * per-view binning launch (k_bin_view) writes on the CUs its view workgroups leave idle, for a
 * K = 1 forward of N views of F faces (mode 0: mr_rasterize_meshes[_world] fragments, 1: the
 * fused render); k_tile_raster writes the rest. */
int64_t mr_binning_background_pixels(int64_t N, int64_t F, int32_t H, int32_t W, int32_t mode);

/* grad_face_verts (F,3,3) is overwritten (zeroed then accumulated). Any of grad_zbuf, grad_bary,
 * grad_dists may be NULL (PyTorch passes None for an output the loss did not use): it counts as
 * zero, and no zero-filled tensor needs to be allocated for it. */
int32_t mr_rasterize_meshes_backward(const float* face_verts, const int64_t* pix_to_face,
                                     const float* grad_zbuf, const float* grad_bary, const float* grad_dists,
                                     int64_t num_meshes, int64_t total_faces, const mr_raster_settings_t* settings,
                                     float* grad_face_verts, void* stream);

/* ---------------- projection (MeshRasterizer.transform) ---------------- */
/* face_verts[n*F + f][c] = ndc(view n, verts[faces[f][c]]) for n < N. */
int32_t mr_project_faces(const float* verts, int64_t V, const int32_t* faces, int64_t F,
                         const mr_view_t* views, int64_t N, float* face_verts, void* stream);
/* grad_verts (V,3) and grad_views (N,12: dR row-major, dT) are overwritten. */
int32_t mr_project_faces_backward(const float* verts, int64_t V, const int32_t* faces, int64_t F,
                                  const int32_t* vadj_ptr, const int32_t* vadj, const mr_view_t* views, int64_t N,
                                  const float* grad_face_verts, float* grad_verts, float* grad_views, void* stream);
/* The same for a batch of N distinct meshes (MeshRasterizer.transform of a Meshes of different
 * meshes, renderer.py:78-80): verts / faces are their union (see mr_mesh_t), view n projects only
 * mesh n's faces [view_face_first[n], view_face_first[n+1]) into face_verts rows of the same ids
 * (the packed order). The backward walks view n's own vertices [view_vert_first[n],
 * view_vert_first[n+1]); max_view_faces / max_view_verts are the largest per-mesh counts. */
int32_t mr_project_faces_meshes(const float* verts, int64_t V, const int32_t* faces, int64_t F,
                                const int64_t* view_face_first, int64_t max_view_faces, const mr_view_t* views,
                                int64_t N, float* face_verts, void* stream);
int32_t mr_project_faces_meshes_backward(const float* verts, int64_t V, const int32_t* faces, int64_t F,
                                         const int32_t* vadj_ptr, const int32_t* vadj, const int64_t* view_vert_first,
                                         int64_t max_view_verts, const mr_view_t* views, int64_t N,
                                         const float* grad_face_verts, float* grad_verts, float* grad_views,
                                         void* stream);

/* ---------------- camera poses (DifferentiableRenderer._camera_pose_from_opencv_to_pytorch) ---------------- */
/* torch_renderer.py:73-80: R_p3d = R_cv^T with columns 0,1 negated; T = t_cv with entries 0,1 negated.
 * views[n] = {R_p3d row-major, T, intr[n]} (bitwise what the torch conversion + packing gives).
 * *_stride = elements between consecutive views (0 broadcasts one pose / one intrinsics row). */
int32_t mr_views_from_opencv(const float* R_cv, int64_t R_stride, const float* t_cv, int64_t t_stride,
                             const float* intr, int64_t intr_stride, int64_t N, mr_view_t* views, void* stream);
/* Chain rule of the conversion above: grad_views (N,12: dR_p3d row-major, dT) -> grad_R_cv (N,3,3),
 * grad_t_cv (N,3), both overwritten. */
int32_t mr_view_grads_to_opencv(const float* grad_views, int64_t N, float* grad_R_cv, float* grad_t_cv, void* stream);

/* ---------------- mesh helpers ---------------- */
/* Meshes.verts_normals_packed: n_f = (v2-v1) x (v0-v1), summed in (corner, face) order, normalized (eps 1e-6).
 * vnormals_raw (V,3) keeps the unnormalized sums for the backward. */
int32_t mr_vertex_normals(const float* verts, int64_t V, const int32_t* faces, int64_t F, const int32_t* vadj_ptr,
                          const int32_t* vadj, float* vnormals, float* vnormals_raw, void* stream);

/* ---------------- fused render (one raster pass -> depth, silhouette, rgb) ---------------- */
size_t mr_render_workspace(int64_t N, int64_t F, int32_t H, int32_t W, int32_t max_faces_per_bin);
/* The same for N distinct meshes of F faces in total (mr_mesh_t.view_face_first set). */
size_t mr_render_workspace_meshes(int64_t N, int64_t F, int32_t H, int32_t W, int32_t max_faces_per_bin);
/* Outputs (each optional per out_flags): depth (N,H,W), silhouette (N,H,W), rgb (N,H,W,C);
 * pix_to_face32 (N,H,W) int32 packed face id n*F+f (distinct meshes: the union face id) or -1 — optional (NULL: not written; the
 * backward does not need it: the workspace keeps each non-empty 8x8 tile's winners and their fragments).
 * cam_centers (Nc,3) world-space specular camera centres, Nc in {1, N}. */
int32_t mr_render_forward(const mr_mesh_t* mesh, const mr_view_t* views, int64_t N, const float* cam_centers,
                          int64_t num_cam_centers, const mr_raster_settings_t* rs, const mr_shade_params_t* sp,
                          float* depth, float* silhouette, float* rgb, int32_t* pix_to_face32, void* workspace,
                          size_t workspace_bytes, void* stream);
/* OpenCV camera poses as DifferentiableRenderer takes them (torch_renderer.py:73-80): R_cv (N,3,3),
 * t_cv (N,3), intrinsics rows {ax, bx, ay, by} (N,4); *_stride = floats between consecutive views
 * (0 broadcasts one row). */
typedef struct mr_opencv_poses {
  const float* R;
  int64_t R_stride;
  const float* t;
  int64_t t_stride;
  const float* intr;
  int64_t intr_stride;
} mr_opencv_poses_t;
/* mr_render_forward for OpenCV poses: the pose conversion (mr_views_from_opencv) happens inside the
 * forward's first launch, which also writes the converted records to views_out (N) for the backward
 * (mr_render_backward_opencv). Replaces DifferentiableRenderer._camera_pose_from_opencv_to_pytorch +
 * the render call (torch_renderer.py:73-80, :110-121, :155-159). */
int32_t mr_render_forward_opencv(const mr_mesh_t* mesh, const mr_opencv_poses_t* poses, mr_view_t* views_out,
                                 int64_t N, const float* cam_centers, int64_t num_cam_centers,
                                 const mr_raster_settings_t* rs, const mr_shade_params_t* sp, float* depth,
                                 float* silhouette, float* rgb, int32_t* pix_to_face32, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* mr_render_forward for PyTorch3D-convention poses given as strided device arrays (R (N,3,3), T (N,3),
 * intr (N,4); a batch stride of 0 broadcasts one row): the view records are packed by the forward's
 * first launch and written to views_out (N) for mr_render_backward — no host-side packing of R, T and
 * intr (upstream MeshRenderer(meshes, R=, T=) callers: camera_pose_optimizer.py:248-250,
 * mesh_deformer.py:197). */
int32_t mr_render_forward_poses(const mr_mesh_t* mesh, const mr_poses_t* poses, mr_view_t* views_out, int64_t N,
                                const float* cam_centers, int64_t num_cam_centers, const mr_raster_settings_t* rs,
                                const mr_shade_params_t* sp, float* depth, float* silhouette, float* rgb,
                                int32_t* pix_to_face32, void* workspace, size_t workspace_bytes, void* stream);
/* Backward from upstream grads (each may be NULL when not requested in out_flags).
 * Writes grad_verts (V,3), grad_views (N,12), grad_vcolors (V,3; tex_kind 1 only, may be NULL).
 * `fwd_workspace` must be the one passed to the matching mr_render_forward: its face records and
 * covered-pixel list are reused (nothing is re-rasterized). */
/* The caller's renderers often shade the SAME raster several times per step (camera_pose_optimizer.py:
 * 244,248,250: rasterizer zbuf, silhouette and Phong renders of identical meshes / R / T / cameras /
 * settings). mr_render_reshade shades again from a workspace a previous mr_render_forward[_opencv]
 * filled for the same mesh geometry, views (`views` = that call's view records), sizes and raster
 * settings: it skips projection, binning and rasterization (the winners, face records and fragments
 * are reused) and runs vertex normals (when needed) -> this call's shading records (out_flags slot,
 * MR_SREC_SLOT(k), k != the slots of the other calls still to be differentiated) -> background ->
 * covered pixels. Outputs bitwise those of a full mr_render_forward with the same arguments. Its
 * backward is mr_render_backward[_opencv] over the same workspace with the same out_flags slot. */
int32_t mr_render_reshade(const mr_mesh_t* mesh, const mr_view_t* views, int64_t N, const float* cam_centers,
                          int64_t n_cam_centers, const mr_raster_settings_t* s, const mr_shade_params_t* sp,
                          float* depth, float* sil, float* rgb, int32_t* pix_to_face, void* workspace,
                          size_t workspace_bytes, void* stream);

size_t mr_render_backward_workspace(int64_t N, int64_t V, int64_t F, int32_t H, int32_t W);
int32_t mr_render_backward(const mr_mesh_t* mesh, const float* vnormals_raw, const mr_view_t* views, int64_t N,
                           const float* cam_centers, int64_t num_cam_centers, const mr_raster_settings_t* rs,
                           const mr_shade_params_t* sp, const float* grad_depth,
                           const float* grad_silhouette, const float* grad_rgb, const void* fwd_workspace,
                           void* bwd_workspace, size_t bwd_workspace_bytes, float* grad_verts, float* grad_views,
                           float* grad_vcolors, void* stream);
/* Same as mr_render_backward for views built by mr_views_from_opencv: the per-view pose
 * gradients are written straight in the OpenCV frame, grad_R_cv (N,3,3) and grad_t_cv (N,3)
 * (the chain rule of mr_view_grads_to_opencv fused into the reduction; torch_renderer.py:73-80). */
int32_t mr_render_backward_opencv(const mr_mesh_t* mesh, const float* vnormals_raw, const mr_view_t* views, int64_t N,
                                  const float* cam_centers, int64_t num_cam_centers, const mr_raster_settings_t* rs,
                                  const mr_shade_params_t* sp, const float* grad_depth,
                                  const float* grad_silhouette, const float* grad_rgb, const void* fwd_workspace,
                                  void* bwd_workspace, size_t bwd_workspace_bytes, float* grad_verts,
                                  float* grad_R_cv, float* grad_t_cv, float* grad_vcolors, void* stream);

/* ---------------- soft shading over stored fragments (K >= 1) ---------------- */
/* SoftPhongShader (out_flags = MR_OUT_RGB: phong_shading + softmax_rgb_blend) or SoftSilhouetteShader
 * (MR_OUT_SIL: sigmoid_alpha_blend, rgb = 1) applied to the fragments of mr_rasterize_meshes
 * (pix_to_face (N,H,W,K) packed ids n*F + f of ONE mesh shared by the N views, zbuf, bary
 * (original-face barycentrics), dists). rgba (N,H,W,4) is written. The workspace holds per-face
 * shading records and must be passed unchanged to the backward. */
size_t mr_shade_fragments_workspace(int64_t F);
int32_t mr_shade_fragments_forward(const mr_mesh_t* mesh, const int64_t* pix_to_face, const float* zbuf,
                                   const float* bary, const float* dists, int64_t N, int32_t H, int32_t W, int32_t K,
                                   const float* cam_centers, int64_t num_cam_centers, const mr_shade_params_t* sp,
                                   float* rgba, void* workspace, size_t workspace_bytes, void* stream);
/* Backward from grad_rgba (N,H,W,4): grad_zbuf / grad_dists (N,H,W,K), grad_bary (N,H,W,K,3) (for
 * mr_rasterize_meshes_backward), grad_verts (V,3) of the attribute path (interpolated world positions and
 * vertex normals), grad_vcolors (V,3; tex_kind 1), grad_tex_rgba (Ht,Wt,4) and grad_verts_uvs
 * (num_verts_uvs,2) (tex_kind 2; either may be NULL). All are overwritten. Gradients that are zero by
 * construction may be NULL: grad_zbuf and grad_bary with MR_OUT_SIL (the silhouette blend reads only
 * the distances), grad_zbuf and grad_dists with MR_OUT_HARD (hard_rgb_blend reads neither). */
size_t mr_shade_fragments_backward_workspace(int64_t V, int64_t F);
int32_t mr_shade_fragments_backward(const mr_mesh_t* mesh, const float* vnormals_raw, const int64_t* pix_to_face,
                                    const float* zbuf, const float* bary, const float* dists, int64_t N, int32_t H,
                                    int32_t W, int32_t K, const float* cam_centers, int64_t num_cam_centers,
                                    const mr_shade_params_t* sp, const float* grad_rgba, const void* fwd_workspace,
                                    void* bwd_workspace, size_t bwd_workspace_bytes, float* grad_zbuf,
                                    float* grad_bary, float* grad_dists, float* grad_verts, float* grad_vcolors,
                                    float* grad_tex_rgba, float* grad_verts_uvs, int64_t num_verts_uvs,
                                    void* stream);

/* MeshRenderer(MeshRasterizer(faces_per_pixel = K, 2 <= K <= 64), SoftSilhouetteShader(sigma)) for ONE
 * mesh shared by N views (deform_mesh_with_color.py:153-165) in one pass: the K-deep fragments are blended
 * as they are produced and never written. rgba (N,H,W,4) must hold the background (1, 1, 1, 0) on entry
 * (tiles no face reaches are not written); it gets (1, 1, 1, 1 - prod_k (1 - sigmoid(-d_k / sigma))),
 * bitwise mr_rasterize_meshes_world + mr_shade_fragments_forward(MR_OUT_SIL). views_out / face_verts as
 * mr_rasterize_meshes_world. The workspace keeps each tile's fragments compactly for the backward, which
 * writes grad_face_verts (N*F,3,3) for mr_project_faces_backward: the chain of
 * mr_shade_fragments_backward(MR_OUT_SIL) and mr_rasterize_meshes_backward without fragment-gradient
 * tensors. MR_EUNSUPPORTED for grids the per-view binning does not take (the caller then runs the
 * two-step path). */
size_t mr_soft_silhouette_workspace(int64_t N, int64_t F, int32_t H, int32_t W, int32_t K, int32_t max_faces_per_bin);
int32_t mr_soft_silhouette_forward(const float* verts, int64_t V, const int32_t* faces, int64_t F,
                                   const mr_poses_t* poses, int64_t N, const mr_raster_settings_t* s, float sigma,
                                   mr_view_t* views_out, float* face_verts, float* rgba, void* workspace,
                                   size_t workspace_bytes, void* stream);
int32_t mr_soft_silhouette_backward(const float* face_verts, int64_t N, int64_t F, const mr_raster_settings_t* s,
                                    float sigma, const float* grad_rgba, const void* workspace, float* grad_face_verts,
                                    void* stream);

/* ---------------- instrumentation ---------------- */

/* camera_pose_optimizer.py:257-276 Model.calc_loss fused: sil_loss =
 * L1Loss(sil, mask), hloss = HuberLoss(delta)(depth[mask], depth_ref[mask]), color_loss =
 * MSELoss(rgb, rgb_ref); out[4] = {sil_loss + hloss + w_color * color_loss, sil_loss, hloss,
 * color_loss} (device). All inputs hold npix = N*H*W pixels; rgb may be an RGBA view
 * (rgb_stride 4); mask is a bool (uint8) tensor. Deterministic (fixed-order reductions). The
 * backward writes dL/d{depth, sil, rgb (npix,3)} given the device scalar dL/dtotal and the
 * forward's workspace. */
size_t mr_pose_loss_workspace(int64_t npix);
int32_t mr_pose_loss_forward(const float* depth, const float* sil, int64_t sil_stride, const float* rgb,
                             int64_t rgb_stride, const uint8_t* mask, const float* depth_ref, const float* rgb_ref,
                             int64_t npix, float delta, float w_color, float* out, void* ws, size_t ws_bytes,
                             void* stream);
/* sil_stride 1: sil is (npix); 4: sil is channel 3 of an (npix, 4) RGBA tensor (the SoftSilhouetteShader
 * image the reference slices with [..., 3]), read in place. rgb_stride 3 or 4 likewise. The gradients
 * come back in the same layouts, for the whole tensors the views were taken from: g_sil (npix) or
 * (npix, 4) RGBA with zero RGB, g_rgb (npix, 3) or (npix, 4) with zero alpha — what the slices'
 * backward would produce, without its zero-filled buffer and strided copy. */
int32_t mr_pose_loss_backward(const float* depth, const float* sil, int64_t sil_stride, const float* rgb,
                              int64_t rgb_stride, const uint8_t* mask, const float* depth_ref, const float* rgb_ref,
                              int64_t npix, float delta, float w_color, const float* g_total, const void* fwd_ws,
                              float* g_depth, float* g_sil, float* g_rgb, void* stream);
/* The forward that also writes the gradients for dL/dtotal = 1 (same layouts as mr_pose_loss_backward):
 * the loss is linear in dL/dtotal, so one pass over the inputs serves both directions;
 * mr_pose_loss_scale then multiplies the three buffers by the device scalar dL/dtotal in place (a no-op
 * grid when it is 1). total (1 float) and terms (3: sil_loss, hloss, color_loss) are separate outputs;
 * the gradient buffers are all three or all NULL (the loss alone); RGBA gradient buffers 16-B aligned. */
int32_t mr_pose_loss_forward_grad(const float* depth, const float* sil, int64_t sil_stride, const float* rgb,
                                  int64_t rgb_stride, const uint8_t* mask, const float* depth_ref, const float* rgb_ref,
                                  int64_t npix, float delta, float w_color, float* total, float* terms, void* ws,
                                  size_t ws_bytes, float* g_depth, float* g_sil, float* g_rgb, void* stream);
int32_t mr_pose_loss_scale(const float* g_total, int64_t npix, int64_t sil_stride, int64_t rgb_stride, float* g_depth,
                           float* g_sil, float* g_rgb, void* stream);

/* upstream pytorch3d.transforms.quaternion_to_matrix (camera_pose_optimizer.py:241: the 7-vector
 * pose's real-first quaternion, not renormalised: two_s = 2 / |q|^2) for N quaternions q (rows
 * q_stride floats apart) -> R (N,3,3), torch's operation order (bitwise the elementwise torch
 * formula); the backward writes dL/dq (N,4) from dL/dR. One launch each instead of ~90 tiny torch
 * kernels per optimiser step. */
int32_t mr_quaternion_to_matrix(const float* q, int64_t q_stride, int64_t N, float* R, void* stream);
int32_t mr_quaternion_to_matrix_backward(const float* q, int64_t q_stride, const float* grad_R, int64_t N,
                                         float* grad_q, void* stream);

/* Mesh shape priors of a packed batch of meshes (PyTorch3D mesh_edge_loss, mesh_laplacian_smoothing(method=
 * "uniform"), mesh_normal_consistency; deform_mesh_with_color.py:248-256, mesh_deformer.py:314-320) in one
 * forward pass and one gathering backward. Every loss is sum(weight * term) with the weights 1 / (elements of
 * that kind in the element's mesh * meshes) supplied by the caller:
 *   edge       per unique edge (v0, v1):                (|v0 - v1| - target_length)^2
 *   Laplacian  per vertex i with neighbours N(i):       |mean_{j in N(i)} v_j - v_i|   (-v_i when isolated)
 *   normal     per pair of faces sharing edge (e0, e1), opposite vertices a, b:
 *              1 - n0.n1 / (max(|n0|, 1e-8) max(|n1|, 1e-8)), n0 = (e1-e0) x (a-e0), n1 = -(e1-e0) x (b-e0)
 * Topology (device, int32, built once per faces tensor by the caller): edges (E,2); nbr_ptr (V+1) / nbr (2E), the
 * CSR of each vertex's neighbours; pairs (P,4) = e0, e1, a, b; pair_ptr (V+1) / pair_idx (4P), the CSR of each
 * vertex's entries 4 * pair + role (role = its column in `pairs`). vert_w is (V,2): the vertex's Laplacian weight
 * and the edge weight of its mesh. `terms` is a mask of MR_PRIOR_*; out[3] = edge, Laplacian, normal loss
 * (device floats, 0 for a term left out). want_grad != 0 also leaves in the workspace what the backward
 * gathers. The backward writes grad_verts (V,3) with plain stores, scaled by the device scalars g_edge / g_lap /
 * g_norm (NULL: that loss was not differentiated); no atomics, bitwise reproducible. `terms` and the sizes must be
 * those of the forward. mr_mesh_priors_workspace returns 0 when a size is out of range. */
enum { MR_PRIOR_EDGE = 1, MR_PRIOR_LAPLACIAN = 2, MR_PRIOR_NORMAL = 4, MR_PRIOR_ALL = 7 };
size_t mr_mesh_priors_workspace(int64_t V, int64_t E, int64_t P);
int32_t mr_mesh_priors_forward(const float* verts, int64_t V, const int32_t* edges, const float* edge_w, int64_t E,
                               const int32_t* nbr_ptr, const int32_t* nbr, const float* vert_w, const int32_t* pairs,
                               const float* pair_w, int64_t P, float target_length, int32_t terms, int32_t want_grad,
                               float* out, void* ws, size_t ws_bytes, void* stream);
int32_t mr_mesh_priors_backward(const float* verts, int64_t V, const int32_t* nbr_ptr, const int32_t* nbr,
                                const float* vert_w, const int32_t* pair_ptr, const int32_t* pair_idx, int64_t E,
                                int64_t P, float target_length, int32_t terms, const float* g_edge, const float* g_lap,
                                const float* g_norm, const void* fwd_ws, float* grad_verts, void* stream);

/* Point clouds (PyTorch3D chamfer_distance with its K = 1 nearest neighbours; mesh_deformer.py:299-352,
 * deform_mesh_from_pcd.py:160-212, chamfer_loss_evaluation.py:126). x (N,P1,3), y (N,P2,3) float32 on the device;
 * x_lengths / y_lengths (N) int64 device arrays or NULL (every cloud full; values are clamped to [0, P]).
 * The distance is float32 in a fixed order without FMA: norm 2 (dx*dx + dy*dy) + dz*dz, norm 1 (|dx| + |dy|) + |dz|;
 * equal distances resolve to the lowest target index. mr_nearest_points writes, for every point of x its nearest
 * point of y (dist_x, idx_x (N,P1)) and the reverse (dist_y, idx_y (N,P2)); entries past a length, or of a cloud
 * whose counterpart has length 0, are 0 / -1. Coordinates must be finite.
 *
 * mr_chamfer_forward: out = the loss ((N) floats without a batch-reduction flag, else 1 float): per cloud
 * weights[n] * (sum of its points' distances, divided by max(length, 1) with MR_CHAMFER_POINT_MEAN), x -> y plus
 * y -> x (x -> y alone with MR_CHAMFER_SINGLE); summed over the batch with MR_CHAMFER_BATCH_SUM, and divided by
 * sum(weights) (N without weights; the loss is 0 when that sum is 0) with MR_CHAMFER_BATCH_MEAN. weights (N) may be
 * NULL. idx_x / idx_y (may be NULL) and coef (2,N; may be NULL) are what the backward reads. All sums run in a fixed
 * order; nothing is read back by the host. mr_chamfer_backward writes grad_x (N,P1,3) and grad_y (N,P2,3) for the
 * upstream gradient grad_out (device: (N) without a batch-reduction flag, else 1 float); the many-to-one part is
 * summed with 64-bit fixed-point integer atomics, so the result is bitwise reproducible (differences of
 * magnitude >= 2^24 take float atomics). norm and flags must be those of the forward. The *_workspace queries
 * return 0 when a size is out of range. */
enum { MR_CHAMFER_POINT_MEAN = 1, MR_CHAMFER_BATCH_MEAN = 2, MR_CHAMFER_BATCH_SUM = 4, MR_CHAMFER_SINGLE = 8,
       MR_CHAMFER_ALL = 15 };
size_t mr_nearest_points_workspace(int64_t N, int64_t P1, int64_t P2);
int32_t mr_nearest_points(const float* x, const float* y, int64_t N, int64_t P1, int64_t P2, const int64_t* x_lengths,
                          const int64_t* y_lengths, int32_t norm, float* dist_x, int32_t* idx_x, float* dist_y,
                          int32_t* idx_y, void* ws, size_t ws_bytes, void* stream);
size_t mr_chamfer_workspace(int64_t N, int64_t P1, int64_t P2);
int32_t mr_chamfer_forward(const float* x, const float* y, int64_t N, int64_t P1, int64_t P2, const int64_t* x_lengths,
                           const int64_t* y_lengths, const float* weights, int32_t norm, int32_t flags, int32_t* idx_x,
                           int32_t* idx_y, float* coef, float* out, void* ws, size_t ws_bytes, void* stream);
size_t mr_chamfer_backward_workspace(int64_t N, int64_t P1, int64_t P2);
int32_t mr_chamfer_backward(const float* x, const float* y, int64_t N, int64_t P1, int64_t P2, int32_t norm,
                            int32_t flags, const int32_t* idx_x, const int32_t* idx_y, const float* coef,
                            const float* grad_out, float* grad_x, float* grad_y, void* ws, size_t ws_bytes,
                            void* stream);

/* Points on the faces of a packed batch of meshes (PyTorch3D sample_points_from_meshes after its random draws):
 * verts (V,3), faces (F,3) int32 over packed vertex ids, face_idx (M) packed face ids, uv (2,M) in [0,1).
 * points[m] = (w0 a + w1 b) + w2 c with s = sqrt(u), w0 = 1 - s, w1 = s (1 - v), w2 = s v over face face_idx[m]'s
 * corners a, b, c; zeros for a negative id (a mesh without faces). The backward sums w_k * grad_points[m] into the
 * three vertices (grad_verts (V,3)) with the fixed-point atomics of mr_chamfer_backward (bitwise reproducible;
 * resolution 2^-32 absolute). mr_face_areas: areas[f] = 0.5 |(b - a) x (c - a)|. */
int32_t mr_sample_points_forward(const float* verts, int64_t V, const int32_t* faces, int64_t F,
                                 const int32_t* face_idx, const float* uv, int64_t M, float* points, void* stream);
size_t mr_sample_points_backward_workspace(int64_t V);
int32_t mr_sample_points_backward(int64_t V, const int32_t* faces, int64_t F, const int32_t* face_idx, const float* uv,
                                  int64_t M, const float* grad_points, float* grad_verts, void* ws, size_t ws_bytes,
                                  void* stream);
int32_t mr_face_areas(const float* verts, int64_t V, const int32_t* faces, int64_t F, float* areas, void* stream);

/* Similarity alignment of point clouds (PyTorch3D corresponding_points_alignment and iterative_closest_point;
 * pytorch3d_icp_registeration.py:154-185). A cloud's transform is 13 floats "rts": R (3x3, row-major), T (3), s,
 * with y = s (x R) + T for row vectors, evaluated in float32 in that order without FMA.
 *
 * mr_points_alignment: rts (N,13) = the transform that takes x (N,P,3) to y (N,P,3) in the weighted least-squares
 * sense. weights (N,P) >= 0 or NULL (ones); lengths (N) or NULL: points past a cloud's length weigh 0. Means,
 * covariance (sum w (x - mx)(y - my)^T / max(sum w, eps)) and the 3x3 SVD (one-sided Jacobi, a fixed number of
 * sweeps) are float64 and summed in a fixed order; R = U E V^T with E = diag(1, 1, det(U V^T)), or the identity with
 * MR_ICP_ALLOW_REFLECTION; s = tr(E S) / max(sum w |x - mx|^2 / sum w, eps) with MR_ICP_ESTIMATE_SCALE, else 1;
 * T = my - s mx R. A cloud whose weights sum to 0 gets the identity.
 *
 * ICP of x (N,P1,3) onto y (N,P2,3): mr_icp_init sets rts to (R0 (N,3,3), T0 (N,3), s0 (N)) or, all three NULL, the
 * identity, clears status and prepares the workspace. mr_icp_iterate then enqueues `iterations` iterations without
 * synchronising: nearest target (squared L2, lowest index on ties, within y_lengths) of every transformed source
 * point; alignment of the ORIGINAL x to those targets (x_lengths as weights, eps 1e-9) into rts and into slot
 * status[1] of history (max_iterations,N,13); rmse (N) = sqrt(sum |s x R + T - y_nn|^2 / max(length, 1e-9)) under the
 * new transform; rel = (previous rmse - rmse) / previous rmse in float32 (1 on the first iteration). status is two
 * int32 on the device: [0] becomes 1 when rel <= relative_rmse_thr for every cloud (a NaN does not pass), [1] counts
 * the iterations run. Once status[0] is set or status[1] == max_iterations every further kernel returns at once, so
 * the caller may enqueue in batches of any size and read status between them: the results do not depend on the
 * batch size. The same ws, rts, history, rmse and status go to every call of one registration. mr_icp_transform
 * writes out (N,P,3) = s (x R) + T for every entry of x, with the code the iterations use. */
enum { MR_ICP_ESTIMATE_SCALE = 1, MR_ICP_ALLOW_REFLECTION = 2, MR_ICP_ALL = 3 };
size_t mr_icp_workspace(int64_t N, int64_t P1, int64_t P2);
int32_t mr_icp_init(const float* x, int64_t N, int64_t P1, int64_t P2, const int64_t* x_lengths, const float* R0,
                    const float* T0, const float* s0, float* rts, int32_t* status, void* ws, size_t ws_bytes,
                    void* stream);
int32_t mr_icp_iterate(const float* x, const float* y, int64_t N, int64_t P1, int64_t P2, const int64_t* x_lengths,
                       const int64_t* y_lengths, int32_t flags, float relative_rmse_thr, int32_t max_iterations,
                       int32_t iterations, float* rts, float* history, float* rmse, int32_t* status, void* ws,
                       size_t ws_bytes, void* stream);
int32_t mr_icp_transform(const float* x, int64_t N, int64_t P, const float* rts, float* out, void* stream);

/* Point-to-plane ICP: a second estimator on the loop of mr_icp_iterate, rigid (s stays what mr_icp_init set).
 * mr_icp_init and mr_icp_transform are used as they are, with a workspace of mr_icp_plane_workspace bytes (it begins
 * with mr_icp_workspace's layout). y_normals (N,P2,3) are used as given: a zero normal contributes nothing, a
 * normal's sign does not matter. max_dist2 is the float32 square of the maximum correspondence distance, or +inf.
 * Per cloud, with L1, L2 its lengths and (R, T, s) = rts, every iteration:
 *  1. p_i = s (x_i R) + T in float32 (the transform code above), i < L1; j(i) the nearest target j < L2 by the float32
 *     squared distance (dx*dx + dy*dy) + dz*dz, the lowest index on ties (mr_icp_iterate's search). A pair is valid
 *     iff that distance is <= max_dist2 (+inf: every pair); m counts the valid pairs.
 *  2. In float64 and a fixed order: c = s (mx R) + T, mx the mean of the cloud's source points; per valid pair with
 *     q = y_j, n = y_normals_j: r = (p - q).n, J = [(p - c) x n, n] (6); A = sum J J^T, b = sum J r.
 *  3. xi = (w, t) solves (A + lam I) xi = -b, lam = 1e-9 trace(A) / 6, by a 6x6 Cholesky in float64; xi = 0 when
 *     trace(A) is not > 0 (m = 0 included), a pivot is not > 0 or the solution is not finite. E = exp([w]x) by
 *     Rodrigues in float64 (below |w| = 1e-4 the series sin(th)/th = 1 - th^2/6, (1 - cos th)/th^2 = 1/2 - th^2/24).
 *  4. R <- R E^T, T <- (T - c) E^T + c + t (row vectors), s unchanged: formed in float64 from the float32 values and
 *     rounded once to float32, into rts and slot status[1] of history. xi = 0 keeps rts bit for bit.
 *  5. rmse = float32(sqrt(sum_valid ((p'_i - q_i).n_i)^2 / max(m, 1))), p' the float32 transform code with the new
 *     rts; correspondences and validity are this iteration's.
 *  6. rel = (previous rmse - rmse) / previous rmse in float32, 1 on the first iteration; a cloud is done when
 *     rel <= relative_rmse_thr (a NaN does not pass) or m == 0 (it keeps its transform and reports rmse 0).
 *     status[0] becomes 1 when every cloud is done in the same iteration. status words, idle kernels, batching of
 *     the status reads and the independence of the results from the batch size: as mr_icp_iterate.
 * Four launches an iteration, no (N,P1,P2) matrix, no host read. mr_icp_plane_solve_host (host only, no GPU) runs
 * steps 3-4, the code the kernel runs, on one system: A21 the upper triangle of A row by row, b6, rts_in (13),
 * c3 -> rts_out (13). */
size_t mr_icp_plane_workspace(int64_t N, int64_t P1, int64_t P2);
int32_t mr_icp_plane_iterate(const float* x, const float* y, const float* y_normals, int64_t N, int64_t P1, int64_t P2,
                             const int64_t* x_lengths, const int64_t* y_lengths, float max_dist2,
                             float relative_rmse_thr, int32_t max_iterations, int32_t iterations, float* rts,
                             float* history, float* rmse, int32_t* status, void* ws, size_t ws_bytes, void* stream);
int32_t mr_icp_plane_solve_host(const double* A21, const double* b6, const float* rts_in, const double* c3,
                                float* rts_out);
size_t mr_points_alignment_workspace(int64_t N, int64_t P);
int32_t mr_points_alignment(const float* x, const float* y, int64_t N, int64_t P, const int64_t* lengths,
                            const float* weights, int32_t flags, double eps, float* rts, void* ws, size_t ws_bytes,
                            void* stream);

/* The chamfer distance of ONE cloud pair under S poses (the pose-search inner loop of chamfer_loss_evaluation.py:
 * 105-126 and pytorch3d_icp_evaluation.py:158-239): x (P1,3), y (P2,3), rts (S,13) as for ICP above, x' = s (x R) + T
 * with the ICP code's operation order. out[k] (S) is what mr_chamfer_forward without a batch-reduction flag gives
 * for the clouds (x' of pose k, y): flags takes MR_CHAMFER_POINT_MEAN and MR_CHAMFER_SINGLE. One launch whose
 * workgroups each own a pose, a direction and 512 queries and scan every target (x' is formed in registers or while
 * it is staged: it is never written), then a finalising launch; no memset, no atomics, nothing read by the host.
 * idx_x (S,P1) / idx_y (S,P2) (each may be NULL; idx_y is not written with MR_CHAMFER_SINGLE): the neighbours, ties to
 * the lowest index. pose_grad (S,13) or NULL: d out[k] / d (R, T, s) of pose k in rts' layout, from float64 sums in a
 * fixed order (bitwise reproducible). Large clouds under few poses leave most of the chip idle: that case is
 * correct, and mr_chamfer_forward on materialised clouds is the faster call for it. */
size_t mr_posed_chamfer_workspace(int64_t S, int64_t P1, int64_t P2);
int32_t mr_posed_chamfer(const float* x, const float* y, int64_t P1, int64_t P2, const float* rts, int64_t S,
                         int32_t norm, int32_t flags, float* out, int32_t* idx_x, int32_t* idx_y, float* pose_grad,
                         void* ws, size_t ws_bytes, void* stream);

/* Point-to-triangle distances (PyTorch3D point_mesh_face_distance, point_face_distance, face_point_distance) of a
 * packed batch of N meshes and N clouds that pair up one to one: points (P,3) and verts (V,3) float32, faces (T,3)
 * int32 over packed vertex ids; points_first / points_count and faces_first / faces_count (N) int64 device arrays
 * give cloud n's points and mesh n's faces as a range of the packed arrays (a range that does not lie inside its
 * array counts as empty; a face with a vertex id outside [0, V) is skipped). max_points / max_faces: host-side
 * upper bounds of the counts, which size the grids (P and T always serve); the host reads nothing from the device.
 *
 * d(p, tri) for tri = (v0, v1, v2) is the squared distance from p to the closest point of the triangle, float32 in
 * a fixed operation order without FMA, with IEEE division and square root. With n = (v1 - v0) x (v2 - v0) and
 * area = |n| / 2: if area >= min_triangle_area, |n| > 1e-8 and the barycentric coordinates of p's orthogonal
 * projection onto the plane all lie in [0, 1], d = ((v0 - p) . n / |n|)^2. Otherwise d = min(seg(p, v0, v1),
 * seg(p, v1, v2), seg(p, v2, v0)), where seg(p, a, b) = |p - (a + t (b - a))|^2 with t = clamp((p - a) . (b - a) /
 * |b - a|^2, 0, 1), and = |p - b|^2 when |b - a|^2 <= 1e-8. So a triangle below the area threshold is its three
 * edges and a collapsed one a point; finite coordinates never give NaN or Inf (short of float32 overflow).
 * min_triangle_area = 0 gives the true point-to-triangle distance. Equal distances resolve to the lowest index,
 * in both directions.
 *
 * mr_point_face_nearest writes for every point its nearest face of its own mesh (dist_p (P), idx_p (P): the face's
 * index within the mesh) and for every face its nearest point of its own cloud (dist_f (T), idx_f (T): the point's
 * index within the cloud); each output may be NULL. A point whose mesh has no faces and a face whose cloud is
 * empty get 0 / -1. Elements outside every range are not written.
 *
 * mr_point_mesh_face_forward: out[0] = (1/N) sum_n ((1/P_n) sum_p dist_p + (1/T_n) sum_t dist_f); a pair whose
 * cloud or mesh is empty contributes 0. Sums are float64 in a fixed order. idx_p / idx_f (may be NULL) and coef
 * (2,N; may be NULL) are what the backward reads.
 *
 * mr_point_mesh_face_backward writes grad_points (P,3) and grad_verts (V,3): for every winning pair, with c the
 * closest point and b its barycentrics (those of the projection in the plane case; (1 - t, t) on the winning edge
 * and 0 at the third vertex otherwise), dd/dp = 2 (p - c) and dd/dv_i = -2 b_i (p - c), times the pair's weight:
 * coef[direction, n] * grad_out[0] (grad_out: 1 float on the device), or grad_dist_p[point] / grad_dist_f[face]
 * where those per-distance upstream gradients are given (the unreduced functions; coef and grad_out may then be
 * NULL). A NULL idx_p / idx_f leaves that direction out. Everything many-to-one is summed with 64-bit fixed-point
 * integer atomics, so the result is bitwise reproducible. min_triangle_area must be the forward's. The *_workspace
 * queries return 0 when a size is out of range. */
size_t mr_point_face_nearest_workspace(int64_t N, int64_t P, int64_t T);
int32_t mr_point_face_nearest(const float* points, int64_t P, const int64_t* points_first, const int64_t* points_count,
                              int64_t max_points, const float* verts, int64_t V, const int32_t* faces, int64_t T,
                              const int64_t* faces_first, const int64_t* faces_count, int64_t max_faces, int64_t N,
                              float min_triangle_area, float* dist_p, int32_t* idx_p, float* dist_f, int32_t* idx_f,
                              void* ws, size_t ws_bytes, void* stream);
size_t mr_point_mesh_face_workspace(int64_t N, int64_t P, int64_t T);
int32_t mr_point_mesh_face_forward(const float* points, int64_t P, const int64_t* points_first,
                                   const int64_t* points_count, int64_t max_points, const float* verts, int64_t V,
                                   const int32_t* faces, int64_t T, const int64_t* faces_first,
                                   const int64_t* faces_count, int64_t max_faces, int64_t N, float min_triangle_area,
                                   int32_t* idx_p, int32_t* idx_f, float* coef, float* out, void* ws, size_t ws_bytes,
                                   void* stream);
size_t mr_point_mesh_face_backward_workspace(int64_t P, int64_t V);
int32_t mr_point_mesh_face_backward(const float* points, int64_t P, const int64_t* points_first,
                                    const int64_t* points_count, int64_t max_points, const float* verts, int64_t V,
                                    const int32_t* faces, int64_t T, const int64_t* faces_first,
                                    const int64_t* faces_count, int64_t max_faces, int64_t N, float min_triangle_area,
                                    const int32_t* idx_p, const int32_t* idx_f, const float* coef, const float* grad_out,
                                    const float* grad_dist_p, const float* grad_dist_f, float* grad_points,
                                    float* grad_verts, void* ws, size_t ws_bytes, void* stream);

/* Point-cloud rendering (PyTorch3D rasterize_points with naive semantics, alpha_composite, norm_weighted_sum).
 *
 * mr_rasterize_points: points (total_points,3) hold NDC x, NDC y and view z; view n draws rows first[n] ..
 * first[n] + count[n] - 1 (several views may name the same rows). Pixel centres are the mesh rasterizer's. Point p
 * covers a pixel iff z >= 0 and d2 = dx*dx + dy*dy < r*r (float32, dx = x - x_pixel, strict); r = radius, or
 * radius_per_point[row] when that is not NULL. A pixel keeps the K <= 50 covering points of smallest (z, row),
 * ascending: idx (N,H,W,K) = idx_base[n] + (row - first[n]) (idx_base NULL: the row), zbuf, dists = d2; -1 in empty
 * slots. Points with a NaN coordinate are not drawn. No workspace and no capacity: every (view, tile) scans its
 * view's cloud in chunks of mr_point_raster_chunk() points, so the results depend on no setting.
 * mr_rasterize_points_backward: grad_points (total_points,3) += (grad_dists 2 dx, grad_dists 2 dy, grad_zbuf) of every
 * filled slot (either gradient may be NULL), summed with 64-bit fixed-point atomics: bitwise reproducible. */
int32_t mr_point_raster_chunk(void);
int32_t mr_rasterize_points(const float* points, const int64_t* first, const int64_t* count, const int64_t* idx_base,
                            int64_t N, int64_t total_points, int32_t H, int32_t W, float radius,
                            const float* radius_per_point, int32_t K, int64_t* idx, float* zbuf, float* dists,
                            void* stream);
size_t mr_rasterize_points_backward_workspace(int64_t total_points);
int32_t mr_rasterize_points_backward(const float* points, const int64_t* first, const int64_t* idx_base, int64_t N,
                                     int64_t total_points, int32_t H, int32_t W, int32_t K, const int64_t* idx,
                                     const float* grad_zbuf, const float* grad_dists, float* grad_points, void* ws,
                                     size_t ws_bytes, void* stream);

/* PointsRasterizer.transform: view n projects the world points src_first[n] .. + count[n] - 1 of points (rows may be
 * shared between views) to out rows dst_first[n] ..: (ax (x / z) + bx, ay (y / z) + by, z) of X R + T, views (N,16)
 * = R (9), T (3), ax, bx, ay, by, the operand order of mr_project_faces. The backward gives grad_points
 * (total_points,3), summed over the views through fixed-point atomics, and grad_views (N,12) = d / d (R, T) from
 * float64 sums in a fixed order. */
int32_t mr_project_points(const float* points, const int64_t* src_first, const int64_t* dst_first,
                          const int64_t* count, int64_t N, int64_t max_count, const float* views, float* out,
                          void* stream);
size_t mr_project_points_backward_workspace(int64_t total_points);
int32_t mr_project_points_backward(const float* points, const int64_t* src_first, const int64_t* dst_first,
                                   const int64_t* count, int64_t N, int64_t total_points, const float* views,
                                   const float* grad_ndc, float* grad_points, float* grad_views, void* ws,
                                   size_t ws_bytes, void* stream);

/* Compositing of K-deep point fragments: idx / vals (N,H,W,K), feats (P,C), out (N,H,W,C). Slots with idx < 0 are
 * skipped; the feature row of a slot is idx - feat_sub[n] (feat_sub NULL: idx). alpha = vals, or with
 * MR_COMPOSITE_DISTS 1 - vals / r^2 (r = radius, or radius_per_point[idx] of n_radius entries). Default: alpha
 * compositing, out_c = sum_k f_c alpha_k prod_{j<k} (1 - alpha_j); MR_COMPOSITE_NORM: sum_k f_c alpha_k /
 * max(sum_k alpha_k, 1e-4). background (C) or NULL: the colour of every pixel whose first slot is empty. The backward
 * writes grad_vals (N,H,W,K) and grad_feats (P,C), the latter through fixed-point atomics. */
enum { MR_COMPOSITE_NORM = 1, MR_COMPOSITE_DISTS = 2 };
int32_t mr_composite_points_forward(const int64_t* idx, const float* vals, const float* feats, int64_t N, int32_t H,
                                    int32_t W, int32_t K, int32_t C, int64_t P, int32_t flags, float radius,
                                    const float* radius_per_point, int64_t n_radius, const int64_t* feat_sub,
                                    const float* background, float* out, void* stream);
size_t mr_composite_points_backward_workspace(int64_t P, int32_t C);
int32_t mr_composite_points_backward(const int64_t* idx, const float* vals, const float* feats, int64_t N, int32_t H,
                                     int32_t W, int32_t K, int32_t C, int64_t P, int32_t flags, float radius,
                                     const float* radius_per_point, int64_t n_radius, const int64_t* feat_sub,
                                     const float* background, const float* grad_out, float* grad_vals,
                                     float* grad_feats, void* ws, size_t ws_bytes, void* stream);

/* Work counters left in `workspace` by the last mr_render_forward / mr_rasterize_meshes that used it
 * (same N, total faces, H, W, max_faces_per_bin). Synchronises `stream`; for benchmarks and tools.
 * out[0] = (tile, face) list entries, out[1] = raster work units, out[2] = non-empty 8x8 tiles,
 * out[3] = covered pixels. */
/* 1 when a batch of N views with total_faces face instances at H x W takes the per-view binning
 * (k_bin_rect_* -> k_bin_view: tile grids of <= 16,384 8x8 tiles, <= 256 a side), 0 when it takes
 * count -> scan -> fill. The fused soft silhouette and the deterministic face gradients need the former. */
int32_t mr_per_view_binning(int64_t N, int64_t total_faces, int32_t H, int32_t W);

int32_t mr_workspace_stats(const void* workspace, int64_t N, int64_t total_faces, int32_t H, int32_t W,
                           int32_t max_faces_per_bin, int64_t* out, void* stream);

/* The 8 raw work counters at the head of a forward workspace (same sizes as the forward that used
 * it): [0] work units, [1] non-empty tiles, [3] kept soft-silhouette fragments, [4..5] list entries
 * (u64), [6] tiles the K-deep raster walked near-to-far (its depth-ordered list walk). Synchronises
 * `stream`; for tests and tools. */
int32_t mr_workspace_counters(const void* workspace, int64_t N, int64_t total_faces, int32_t H, int32_t W,
                              int32_t max_faces_per_bin, int32_t* out8, void* stream);

/* K nearest neighbours (PyTorch3D knn_points, 1 <= K <= 32; MR_EUNSUPPORTED above). For every point of p1 (N,P1,3)
 * the K smallest (distance, index) pairs over p2[n, :lengths2[n]], ascending, with the distance of the chamfer calls
 * above: equal distances resolve to the lower index, inside the K kept and at the K-th / (K+1)-th boundary. dists
 * (N,P1,K) float32, idx (N,P1,K) int32; slots k >= min(K, lengths2[n]) and rows i >= lengths1[n] are 0 / -1.
 * One launch whose workgroups each own a tile of queries and scan every target of their cloud, the K-deep lists in
 * registers; only when N * query tiles < 256 is the target range cut into <= 16 splits (chosen from the shapes
 * alone), whose sorted partial lists go through the workspace (8 K splits bytes per query) to a merging launch. The
 * result does not depend on the splits. No memset, no atomics; bitwise reproducible. mr_knn_geometry (host only)
 * returns what the launch would use: queries per workgroup, splits, and the targets staged in LDS at a time (each
 * pointer may be NULL).
 *
 * mr_knn_points_backward: for grad_dists (N,P1,K), grad_p1[n,i] = sum_k 2 g (p1[n,i] - p2[n,idx]) and grad_p2[n,j] =
 * -(the sum of those addends over the (i,k) with idx = j); norm 1: g sign(.) for 2 g (.). Slots with idx < 0 add
 * nothing and their g is not read. One memset and two launches; the many-to-one part is summed with 64-bit
 * fixed-point integer atomics (bitwise reproducible; addends of magnitude >= 2^24 take float atomics). */
size_t mr_knn_points_workspace(int64_t N, int64_t P1, int64_t P2, int32_t K);
int32_t mr_knn_points(const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2, const int64_t* lengths1,
                      const int64_t* lengths2, int32_t norm, int32_t K, float* dists, int32_t* idx, void* ws,
                      size_t ws_bytes, void* stream);
size_t mr_knn_points_backward_workspace(int64_t N, int64_t P1, int64_t P2, int32_t K);
int32_t mr_knn_points_backward(const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2,
                               const int64_t* lengths1, const int64_t* lengths2, int32_t norm, int32_t K,
                               const int32_t* idx, const float* grad_dists, float* grad_p1, float* grad_p2, void* ws,
                               size_t ws_bytes, void* stream);
int32_t mr_knn_geometry(int64_t N, int64_t P1, int64_t P2, int32_t K, int32_t* queries_per_group, int32_t* splits,
                        int32_t* lds_chunk);

/* Farthest-point subsampling (PyTorch3D sample_farthest_points) of points (N,P,3). Per cloud n, with L = lengths[n]
 * (NULL: P; clamped to [0, P]) and k_n = min(K_per_cloud[n], L) (K_per_cloud NULL: Kmax; clamped to [0, Kmax]): the
 * first index is start_idx[n] (NULL: 0; clamped into the cloud); every point p < L carries m[p] = +inf; after each
 * selection s, m[p] = min(m[p], d(p, s)) with the float32 squared distance of the chamfer calls above, and the next
 * index is the p < L with the largest m[p], the lowest index among equal values (a selected point stays in the
 * running with m = 0). idx (N,Kmax) int32 and pts (N,Kmax,3) float32, the selected points' coordinates; the slots
 * k >= k_n are -1 / 0. lengths, K_per_cloud and start_idx are int64 (N,) device arrays.
 * One launch, one workgroup per cloud for all of its rounds, nothing between workgroups; no memset, no atomics;
 * bitwise reproducible. Up to 1,024 * 32 points a cloud lives in its workgroup's registers (and, at 32 points a
 * thread, its m values in LDS); above, the points are read from global memory every round and m lives in the
 * workspace (N * P floats): correct, and slow. mr_farthest_points_geometry (host only) returns what the launch would
 * use: threads per workgroup, points per thread (register path: the bucket 1, 2, 4, ..., 32) and whether the cloud is
 * streamed (each pointer may be NULL). MR_EINVAL for NULL or non-positive sizes, MR_EUNSUPPORTED for clouds too
 * large for 32-bit point ids, MR_EWORKSPACE; all before any GPU call. */
int32_t mr_farthest_points_geometry(int64_t N, int64_t P, int64_t Kmax, int32_t* threads, int32_t* points_per_thread,
                                    int32_t* streamed);
size_t mr_farthest_points_workspace(int64_t N, int64_t P, int64_t Kmax);
int32_t mr_farthest_points(const float* points, int64_t N, int64_t P, const int64_t* lengths, const int64_t* K_per_cloud,
                           int64_t Kmax, const int64_t* start_idx, int32_t* idx, float* pts, void* ws, size_t ws_bytes,
                           void* stream);

/* Local coordinate frames of point clouds (PyTorch3D estimate_pointcloud_local_coord_frames; column 0 of a frame is
 * estimate_pointcloud_normals), 2 <= K <= 64 (MR_EINVAL below, MR_EUNSUPPORTED above). For point i < L = lengths[n]
 * (NULL: P; clamped to [0, P]) of points (N,P,3): the neighbourhood is the K smallest (distance, index) pairs over the
 * same cloud, the point itself included, with mr_knn_points' float32 squared distance and tie rule. With
 * d_k = p_k - p_i and m = mean_k d_k, C = (1/K) sum_k (d_k - m)(d_k - m)^T in float32, summed in neighbour order.
 * curvatures (N,P,3) are C's eigenvalues ascending, frames (N,P,3,3) holds in frames[n,i,:,j] the unit eigenvector of
 * the j-th (column 0 the normal, column 2 the main direction), cov (N,P,6; may be NULL) the upper triangle of C as
 * xx, xy, xz, yy, yz, zz. The solve is a fixed-sweep cyclic Jacobi in float32 on C / trace(C): the frames do not
 * depend on the cloud's scale. C = 0 gives curvatures 0 and the identity before the sign step.
 * Signs: with MR_FRAMES_DISAMBIGUATE, columns 0 and 2 are negated iff 2 #{k : (v_x d_kx + v_y d_ky) + v_z d_kz > 0} < K
 * and column 1 becomes cross(column 0, column 2); without, every column's component of largest magnitude is made
 * positive (the lowest axis among equal magnitudes).
 * Rows i >= L, and every row of a cloud with L < K, are zeros in all outputs. P <= K is MR_EINVAL.
 * One launch whose threads each scan their cloud for their queries' neighbours (lists in registers, bucket 8, 16, 32
 * or 64) and solve in place; only when N * query tiles < 256 is the target range cut into <= 16 splits whose sorted
 * partial lists go through the workspace (8 K splits bytes per point) to a launch that merges and solves. The result
 * does not depend on the splits. No memset, no atomics; bitwise reproducible. mr_point_frames_geometry (host only)
 * returns what the launch would use: the bucket, queries per workgroup, splits, and the targets staged in LDS at a
 * time (each pointer may be NULL). All arguments are checked before any GPU call.
 *
 * mr_symmetric_eig3_host (host only, no GPU): the same solver over M symmetric 3x3 matrices given as (M,6) upper
 * triangles; eigenvalues (M,3) ascending, eigenvectors (M,3,3) in columns, signed as without MR_FRAMES_DISAMBIGUATE. */
enum { MR_FRAMES_DISAMBIGUATE = 1 };
int32_t mr_point_frames_geometry(int64_t N, int64_t P, int32_t K, int32_t* bucket, int32_t* queries_per_group,
                                 int32_t* splits, int32_t* lds_chunk);
size_t mr_point_frames_workspace(int64_t N, int64_t P, int32_t K);
int32_t mr_point_frames(const float* points, int64_t N, int64_t P, const int64_t* lengths, int32_t K, int32_t flags,
                        float* curvatures, float* frames, float* cov, void* ws, size_t ws_bytes, void* stream);
int32_t mr_symmetric_eig3_host(const float* cov, int64_t M, float* eigenvalues, float* eigenvectors);

/* Radius neighbourhoods (PyTorch3D ball_query), any K >= 1. For query i < L1 = lengths1[n] of p1 (N,P1,3), with
 * r2 = radius * radius rounded once to float32 and d(i, j) the float32 squared distance of the calls above: walk
 * j = 0 .. lengths2[n] - 1 in index order; every j with d(i, j) < r2 (strict; a nan distance never hits) takes the
 * next free slot until K are full. dists (N,P1,K) float32 holds the hits' d and idx (N,P1,K) int32 their j: the first
 * K in index order, neither the nearest K nor sorted by distance. Free slots and rows i >= L1 are 0 / -1. radius 0
 * hits nothing; a negative or non-finite radius is MR_EINVAL.
 * One launch whose workgroups each own a tile of queries and stream their cloud's targets through LDS; a hit is
 * stored straight to its slot, a wave stops scanning a chunk once all its queries are full and a workgroup stops once
 * all its waves are. Every thread pads its own free slots: no memset, no atomics; bitwise reproducible. Only when
 * N * query tiles < 256 and P2 > 2048 is the target range cut into <= 16 splits (chosen from the shapes alone) and
 * walked by two launches, a counting pass into the workspace (4 splits bytes per query) and a writing pass that
 * starts every split at the sum of the earlier splits' counts; the result does not depend on the splits.
 * mr_ball_query_geometry (host only) returns what the launch would use: queries per workgroup, splits, and the
 * targets staged in LDS at a time (each pointer may be NULL).
 *
 * mr_ball_query_backward: mr_knn_points_backward at norm 2 and any K >= 1 (the same kernels): grad_p1[n,i] =
 * sum_k 2 g (p1[n,i] - p2[n,idx]), grad_p2 its negative summed per target in 64-bit fixed point. Slots with idx < 0
 * add nothing and their g is not read. Three launches and no memset: the fixed-point rows are cleared by a kernel, so
 * a captured HIP graph can be replayed any number of times. All arguments are checked before any GPU call. */
int32_t mr_ball_query_geometry(int64_t N, int64_t P1, int64_t P2, int32_t K, int32_t* queries_per_group,
                               int32_t* splits, int32_t* lds_chunk);
size_t mr_ball_query_workspace(int64_t N, int64_t P1, int64_t P2, int32_t K);
int32_t mr_ball_query(const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2, const int64_t* lengths1,
                      const int64_t* lengths2, float radius, int32_t K, float* dists, int32_t* idx, void* ws,
                      size_t ws_bytes, void* stream);
size_t mr_ball_query_backward_workspace(int64_t N, int64_t P1, int64_t P2, int32_t K);
int32_t mr_ball_query_backward(const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2,
                               const int64_t* lengths1, const int64_t* lengths2, int32_t K, const int32_t* idx,
                               const float* grad_dists, float* grad_p1, float* grad_p2, void* ws, size_t ws_bytes,
                               void* stream);

/* ICP onto a mesh surface: a third estimator on the loop of mr_icp_iterate, rigid (s stays what mr_icp_init set),
 * the point-to-plane step above against the closest points of the meshes' surfaces. x (N,P1,3) with x_lengths; the
 * packed mesh arguments are mr_point_face_nearest's (above): verts (V,3), faces (T,3) int32 over packed vertex ids,
 * faces_first / faces_count (N) int64 device arrays, max_faces a host-side bound of the counts. Meshes may share
 * faces (equal faces_first): the records are per packed face. mr_icp_init (with any P2 >= 1) and mr_icp_transform
 * are used as they are, on a workspace of mr_icp_mesh_workspace bytes (it begins with mr_icp_plane_workspace's
 * layout). mr_icp_mesh_prepare, once after mr_icp_init and before the first iteration, writes every packed face's
 * triangle record for min_triangle_area into the workspace; the mesh must not change until the registration ends.
 * max_dist2 is the float32 square of the maximum correspondence distance, rounded once, or +inf.
 * Per cloud n with L1 points, mesh n with T_n faces, (R, T, s) = rts, every iteration:
 *  1. Search. p_i = s (x_i R) + T in float32 (the transform code above), i < L1; f(i) the face of mesh n with the
 *     smallest d(p_i, tri), d exactly mr_point_face_nearest's distance for min_triangle_area; the lowest face index
 *     wins a tie; a face with a vertex id outside [0, V) is skipped.
 *  2. Closest point and normal, in float32 without FMA, from the winner's pair: q_i = (b0 v0 + b1 v1) + b2 v2 per
 *     component, b the closest point's barycentrics (those of the projection in the plane case; (1 - t, t) on the
 *     winning edge and 0 at the third vertex otherwise). n_i is the triangle's unit normal if the plane branch
 *     returned the distance; otherwise e = p_i - q_i, l = sqrtf((e0 e0 + e1 e1) + e2 e2), n_i = e / l if l > 1e-8,
 *     else 0: the gradient direction of the distance function, which on a shared edge or vertex does not depend on
 *     which of the tied faces won. A zero normal contributes nothing; the sign does not matter. A pair is valid iff
 *     d <= max_dist2 (+inf: every pair); m counts the valid pairs.
 *  3. Update. Steps 2 to 6 of mr_icp_plane_iterate, unchanged, with q_i and n_i in place of y_j and y_normals_j:
 *     float64 A and b about c, lam = 1e-9 trace(A) / 6, the 6x6 Cholesky and Rodrigues, one rounding to float32 into
 *     rts and slot status[1] of history, the point-to-plane rmse of this iteration's valid pairs under the new
 *     transform, the relative-drop test. A cloud with m = 0 (an empty cloud, a mesh without a usable face, no pair
 *     within the distance) keeps its transform bit for bit, reports rmse 0 and counts as done.
 * Status words, idle kernels, batching of the status reads and the independence of the results from the batch size:
 * as mr_icp_iterate. Four launches an iteration (the scan, closest points with the normal equations, the solve with
 * the new residual, the status), no (P1,T) matrix, no host read; not differentiable.
 * mr_icp_mesh_closest runs the scan and the closest-point code once on a prepared workspace, under rts (N,13) or,
 * NULL, on x as it is: dist (N,P1) and face (N,P1; the index within the mesh) as mr_point_face_nearest's dist_p and
 * idx_p (0 / -1 without a face or past the length; each may be NULL), q and normal (N,P1,3; zeros there).
 * mr_icp_mesh_geometry (host only) reports the scan's launch geometry for a batch: the faces a workgroup stages
 * (chunk, between min_chunk and max_chunk) and the workgroups per cloud; each output may be NULL. */
size_t mr_icp_mesh_workspace(int64_t N, int64_t P1, int64_t T);
int32_t mr_icp_mesh_geometry(int64_t N, int64_t P1, int64_t max_faces, int32_t* chunk, int32_t* min_chunk,
                             int32_t* max_chunk, int64_t* groups);
int32_t mr_icp_mesh_prepare(const float* verts, int64_t V, const int32_t* faces, int64_t T, const int64_t* faces_first,
                            const int64_t* faces_count, int64_t max_faces, int64_t N, int64_t P1,
                            float min_triangle_area, void* ws, size_t ws_bytes, void* stream);
int32_t mr_icp_mesh_iterate(const float* x, int64_t N, int64_t P1, const int64_t* x_lengths, int64_t T,
                            const int64_t* faces_first, const int64_t* faces_count, int64_t max_faces, float max_dist2,
                            float relative_rmse_thr, int32_t max_iterations, int32_t iterations, float* rts,
                            float* history, float* rmse, int32_t* status, void* ws, size_t ws_bytes, void* stream);
int32_t mr_icp_mesh_closest(const float* x, int64_t N, int64_t P1, const int64_t* x_lengths, const float* rts,
                            int64_t T, const int64_t* faces_first, const int64_t* faces_count, int64_t max_faces,
                            float* dist, int32_t* face, float* q, float* normal, void* ws, size_t ws_bytes,
                            void* stream);

/* Per-kernel timing with HIP events recorded on each launch's stream (bench.py).
 * enable=1 clears and starts collection; mr_timing_read synchronizes on the
 * recorded events and returns, per kernel id, launches and summed ms. */
int32_t mr_timing_enable(int32_t enable);
int32_t mr_timing_read(int32_t* launches, double* total_ms, int32_t n);
const char* mr_timing_kernel_name(int32_t k);
int32_t mr_timing_kernel_count(void);

/* A uniform-grid index over the targets of a neighbour search, and mr_knn_points through it.
 *
 * mr_point_grid_build sorts p[n, :lengths[n]] (p (N,P,3); lengths NULL: P) into the cells of one uniform grid per
 * cloud, in `grid`, a device buffer of mr_point_grid_bytes(N, P) bytes that holds no pointers. Per cloud: the bounding
 * box lo .. hi of its points; a cell size h > 0 and dims g = (gx, gy, gz) >= 1 chosen on the device, aiming at 4 points
 * a cell in a uniformly filled box, with gx gy gz <= min(max(lengths[n], 1), P, 2^24) and g_a <= 1024; the cell of a
 * point along axis a is clamp(int(floor((p_a - lo_a) * (1 / h))), 0, g_a - 1) in float32. An axis of zero extent has
 * g_a = 1; an empty cloud, coincident points and a cloud with a coordinate that is not finite have one cell (the
 * search then visits every target of that cloud). Four launches, integer atomics, no memset, nothing read back; the
 * order of the targets inside a cell may differ from run to run, and no result depends on it. The workspace is only
 * used during the call. mr_point_grid_describe copies out, per cloud, dims (N,3), origin_cell (N,4) = lo and h, and the
 * largest number of points in one cell (N) into host arrays (each may be NULL); it synchronises `stream`: for tests
 * and tools.
 *
 * mr_knn_points_grid is mr_knn_points, argument for argument and bit for bit in dists and idx, for a `grid` built
 * from these p2 and lengths2: one launch, a query per lane, which visits the cells in cube rings r = 0, 1, ... around
 * the query's own cell (a query outside the box takes the nearest cell) and stops after ring r >= 1 once it holds K
 * neighbours and the K-th distance is strictly below ((r - 2^-6) h)^2 (1 - 2^-18) (norm 1: (r - 2^-6) h (1 - 2^-18)),
 * a lower bound on the float32 distance of every target in the cells beyond, or when the rings cover the grid.
 * `visited` (device, may be NULL) is one counter the caller clears: every workgroup adds the number of (query, target)
 * distances it evaluated. Nothing read from `grid` is trusted for addressing: a grid of other clouds of the same
 * shapes gives wrong neighbours with idx in [-1, P2), never a fault. The workspace is not used but must be given.
 * MR_EINVAL for NULL or non-positive sizes, K < 1 or a norm other than 1 and 2; MR_EUNSUPPORTED for N > 65535, clouds
 * too large for 32-bit point ids and K > 32; MR_EWORKSPACE ("too small") for the grid buffer and the workspaces; all
 * before any GPU call. The *_bytes / *_workspace functions return a multiple of 256, or 0 out of range. */
size_t mr_point_grid_bytes(int64_t N, int64_t P);
size_t mr_point_grid_build_workspace(int64_t N, int64_t P);
int32_t mr_point_grid_build(const float* p, int64_t N, int64_t P, const int64_t* lengths, void* grid, size_t grid_bytes,
                            void* ws, size_t ws_bytes, void* stream);
size_t mr_knn_points_grid_workspace(int64_t N, int64_t P1, int64_t P2, int32_t K);
int32_t mr_knn_points_grid(const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2, const int64_t* lengths1,
                           const int64_t* lengths2, const void* grid, size_t grid_bytes, int32_t norm, int32_t K,
                           float* dists, int32_t* idx, uint64_t* visited, void* ws, size_t ws_bytes, void* stream);
int32_t mr_point_grid_describe(const void* grid, int64_t N, int64_t P, int32_t* dims, float* origin_cell,
                               int32_t* max_cell_count, void* stream);

/* The ICP loops through a point grid of the targets: mr_icp_iterate_grid is mr_icp_iterate, and
 * mr_icp_plane_iterate_grid is mr_icp_plane_iterate, argument for argument and bit for bit in rts, history, rmse and
 * status, with `grid` (a buffer of mr_point_grid_build for these y and y_lengths, grid_bytes >= mr_point_grid_bytes(N,
 * P2)) and `visited` added. The rule is the search of mr_icp_iterate, through the grid, with the same key in `ws`:
 * the first launch of an iteration leaves, per source point, the key of the nearest target that the brute-force scan
 * leaves (the float32 squared distance and the lowest index on ties; for a point whose every distance is +inf or a
 * NaN, distance +inf and index 0); the three other launches, the workspaces (mr_icp_workspace,
 * mr_icp_plane_workspace), mr_icp_init and mr_icp_transform are used as they are, and a registration may change
 * between the two entry points from one call to the next. One source point per lane walks the cells in cube rings as
 * mr_knn_points_grid does with K = 1. With max_dist2 < +inf the plane estimator's walk also stops after ring r >= 1
 * once ((r - 2^-6) h)^2 (1 - 2^-18) > max_dist2: no target beyond the rings can form a valid pair, and a source point
 * without a valid pair contributes nothing whichever target its key names. `visited` (device, may be NULL) is one
 * counter the caller clears: every workgroup of an iteration that is not idle adds the number of (source, target)
 * distances it evaluated. Nothing read from `grid` is trusted for addressing: a grid of other clouds of the same
 * shapes gives wrong correspondences inside the target, never a fault. MR_EINVAL for a NULL grid and for what the
 * siblings refuse (sizes, flags, max_dist2, max_iterations, iterations, NULL pointers); MR_EUNSUPPORTED as the
 * siblings; MR_EWORKSPACE ("too small") for the grid buffer and the workspace; all before any GPU call. */
int32_t mr_icp_iterate_grid(const float* x, const float* y, int64_t N, int64_t P1, int64_t P2, const int64_t* x_lengths,
                            const int64_t* y_lengths, const void* grid, size_t grid_bytes, int32_t flags,
                            float relative_rmse_thr, int32_t max_iterations, int32_t iterations, float* rts,
                            float* history, float* rmse, int32_t* status, uint64_t* visited, void* ws, size_t ws_bytes,
                            void* stream);
int32_t mr_icp_plane_iterate_grid(const float* x, const float* y, const float* y_normals, int64_t N, int64_t P1,
                                  int64_t P2, const int64_t* x_lengths, const int64_t* y_lengths, const void* grid,
                                  size_t grid_bytes, float max_dist2, float relative_rmse_thr, int32_t max_iterations,
                                  int32_t iterations, float* rts, float* history, float* rmse, int32_t* status,
                                  uint64_t* visited, void* ws, size_t ws_bytes, void* stream);

/* Local frames and radius neighbourhoods through a point grid.
 *
 * mr_point_frames_grid is mr_point_frames, bit for bit in curvatures, frames and cov, with `grid` (a buffer of
 * mr_point_grid_build for these points and lengths, grid_bytes >= mr_point_grid_bytes(N, P)) and `visited` added: the
 * cloud is searched against itself through its own grid. One launch, a query per lane: the lane takes entry j of its
 * cloud's cell-ordered targets as its query (so a wave's lanes walk neighbouring cells), walks the rings as
 * mr_knn_points_grid does until its K-th distance is strictly below the ring bound, which leaves the K smallest
 * (distance, index) keys the brute-force scan leaves, and sums and solves in that list's order; lanes j >= lengths[n]
 * write the zero rows j. No index, neighbour or key goes to memory; the workspace is not used but must be given. The
 * checks are mr_point_frames' (2 <= K <= 64, P > K, flags), then a NULL grid (MR_EINVAL) and the sizes of the grid buffer
 * and the workspace (MR_EWORKSPACE, "too small"), all before any GPU call. A grid of other clouds of the same shape
 * gives wrong frames and, because the output row of a lane is the index its grid entry stores (clamped to P - 1), may
 * leave rows unwritten; every address stays in range.
 *
 * mr_ball_query_grid is mr_ball_query, bit for bit in dists and idx, for 1 <= K <= 64 (MR_EUNSUPPORTED above), with
 * `grid` built from these p2 and lengths2, and `visited`. One launch, a query per lane: a target is a hit iff its
 * float32 squared distance is < r2 = radius * radius (strict), and a hit enters the lane's ascending list on the key
 * (index << 32 | distance bits), so the list ends as the K lowest-indexed hits. Cells are visited in no index order, so
 * a full list stops nothing: the walk ends after ring r >= 1 once ((r - 2^-6) h)^2 (1 - 2^-18) > r2, when no target
 * beyond the rings can be a hit, or when the rings cover the grid. A small radius in a large cloud visits a few cells;
 * a radius of the cloud's size visits all of it, one query per lane, and loses to mr_ball_query. The gradient is
 * mr_ball_query_backward, which reads only idx. `visited` as in mr_knn_points_grid; nothing read from `grid` is trusted
 * for addressing (idx stays in [-1, P2)). The *_workspace functions return 256, or 0 out of range (K included). */
size_t mr_point_frames_grid_workspace(int64_t N, int64_t P, int32_t K);
int32_t mr_point_frames_grid(const float* points, int64_t N, int64_t P, const int64_t* lengths, const void* grid,
                             size_t grid_bytes, int32_t K, int32_t flags, float* curvatures, float* frames, float* cov,
                             uint64_t* visited, void* ws, size_t ws_bytes, void* stream);
size_t mr_ball_query_grid_workspace(int64_t N, int64_t P1, int64_t P2, int32_t K);
int32_t mr_ball_query_grid(const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2, const int64_t* lengths1,
                           const int64_t* lengths2, const void* grid, size_t grid_bytes, float radius, int32_t K,
                           float* dists, int32_t* idx, uint64_t* visited, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355R_H */
