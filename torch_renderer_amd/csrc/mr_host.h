// mi355r — Host runtime shared by the library's translation units (mr_raster.hip, mr_priors.hip, mr_points.hip):
// the thread-local error text, the per-kernel timing events, the one launch construct, the stream memset and
// the workspace carver. Host code only. The error text and the timing pool are defined once, in mr_raster.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mi355r.h"

#define MR_HIDDEN __attribute__((visibility("hidden")))

extern MR_HIDDEN __thread char g_err[512];  // mr_last_error()
static inline int set_err(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// ---------------------------------------------------------------------------
// Optional per-kernel timing: HIP events recorded on the launch stream around
// every timed kernel while enabled (bench.py reads them to price the dominant kernel).
// One list of (id, name): mr_timing_kernel_name's table is generated from it.
// ---------------------------------------------------------------------------
#define MR_KERNEL_IDS(X)                        \
  X(KID_BIN_COUNT, "k_bin_count")               \
  X(KID_BIN_SCAN, "k_bin_scan")                 \
  X(KID_BIN_FILL, "k_bin_fill")                 \
  X(KID_TILE_RASTER, "k_tile_raster")           \
  X(KID_SHADE_FRAG, "k_shade<0>")               \
  X(KID_SHADE_RENDER, "k_shade<1>")             \
  X(KID_RASTER_BWD, "k_raster_bwd")             \
  X(KID_RT_VGRAD_B, "k_rt_vgrad_b")             \
  X(KID_VGRAD_B, "k_vgrad_b")                   \
  X(KID_VNORMALS, "k_vertex_normals")           \
  X(KID_PROJECT, "k_project_faces")             \
  X(KID_PROJECT_BWD, "k_project_faces_bwd")     \
  X(KID_SHADE_REC, "k_shade_rec")               \
  X(KID_FILL_FRAG, "k_fill<0>")                 \
  X(KID_RASTER_K, "k_raster_k")                 \
  X(KID_BWD_FUSED, "k_bwd_fused")               \
  X(KID_RT_VGRAD_A, "k_rt_vgrad_a")             \
  X(KID_FRAG_SHADE, "k_frag_shade_fwd")         \
  X(KID_FRAG_SHADE_BWD, "k_frag_shade_bwd")     \
  X(KID_SETUP, "k_setup_zero")                  \
  X(KID_BIN_RECT, "k_bin_rect")                 \
  X(KID_BIN_VIEW, "k_bin_view")                 \
  X(KID_BAND_BUCKET, "k_band_bucket")           \
  X(KID_POSE_LOSS, "k_pose_loss_fused")         \
  X(KID_POSE_LOSS_SCALE, "k_pose_loss_scale")   \
  X(KID_UNIT_ORDER, "k_unit_order")
#define MR_KID_ENUM(id, name) id,
enum KernelId { KID_NONE = -1, MR_KERNEL_IDS(MR_KID_ENUM) KID_COUNT };  // KID_NONE: an untimed launch
#undef MR_KID_ENUM

#define MR_TPOOL 4096
struct TimingPool {
  int enabled;
  int created;
  hipEvent_t ev[2 * MR_TPOOL];
  int kid[MR_TPOOL];
  int used;
  int dropped;
};
extern MR_HIDDEN TimingPool g_t;

static inline int timing_begin(hipStream_t st) {
  if (!g_t.enabled || g_t.used >= MR_TPOOL) {
    if (g_t.enabled) g_t.dropped++;
    return -1;
  }
  const int i = g_t.used++;
  (void)hipEventRecord(g_t.ev[2 * i], st);
  return i;
}
static inline void timing_end(int i, int kid, hipStream_t st) {
  if (i < 0) return;
  g_t.kid[i] = kid;
  (void)hipEventRecord(g_t.ev[2 * i + 1], st);
}

// One kernel launch: kernel<<<grid, block, lds, st>>>(args...), between timing events under `kid` (KID_NONE:
// none). MR_OK, or MR_ELAUNCH with "<name>: <HIP's error>" as the error text. The arguments travel by
// reference, so a parameter struct is copied once, into the launch. (An overloaded kernel name needs its
// parameter types spelled: launch<ViewBinParams>(...).)
template <typename... KArgs, typename... Args>
static inline int launch(int kid, const char* name, void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds,
                         hipStream_t st, const Args&... args) {
  const int ti = kid >= 0 ? timing_begin(st) : -1;
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  timing_end(ti, kid, st);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MR_OK : set_err(MR_ELAUNCH, "%s: %s", name, hipGetErrorString(e));
}

static inline int memset_async(void* p, int value, size_t bytes, hipStream_t st) {
  return hipMemsetAsync(p, value, bytes, st) == hipSuccess ? MR_OK : set_err(MR_ELAUNCH, "memset failed");
}

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// A workspace layout: fields taken in order from `base` (NULL for a size query; `off` is then the size).
struct Carver {
  char* base;
  size_t off;
  explicit Carver(const void* b, size_t start = 0) : base((char*)b), off(start) {}
  // n elements with nothing after them: the next field follows directly (one memset over both)
  template <typename T> T* take_packed(size_t n) {
    T* p = (T*)(base + off);
    off += sizeof(T) * n;
    return p;
  }
  // n elements, the next field at the following multiple of 256 B
  template <typename T> T* take(size_t n) {
    T* p = take_packed<T>(n);
    off = align_up(off, 256);
    return p;
  }
};
