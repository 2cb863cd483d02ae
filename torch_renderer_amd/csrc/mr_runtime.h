// mi355r — The raster's workspace: batch geometry, the carve (face records, tile lists, work units, per-slot
// winners) and its counters. The host runtime every translation unit shares is mr_host.h.
// Part of mr_raster.hip (included there, in this order).
#pragma once

#define MR_TS 8         // raster tile edge: one 64-lane wave per 8x8 tile (lane = pixel)
#define MR_BT 32        // tile edge of the modular (fragments) backward
#define MR_HT 512       // LDS hash slots in the backward
#define MR_BIN_FPT 2     // faces per thread in the world-space binning kernels
#define MR_LDS_HIST 16384  // per-view tiles binned through an LDS histogram (else global atomics)

// ---------------------------------------------------------------------------
// Workspace: face records, per-(view, 8x8 tile) face lists (count -> scan ->
// fill), work units, compact per-tile depth keys, and (fused path) the compact
// per-view list of covered (pixel, face) pairs.
// ---------------------------------------------------------------------------
#ifndef MR_BANDS_MAX
#define MR_BANDS_MAX 64  // per-view binning: workgroups (bands of tile rows) per view (32 -> 64: C5 k_bin_view 24.6 -> 18.8 us, r6n)
#endif
#define MR_SREC_SLOTS 4  // ShadeRec sets per fused-forward workspace (out_flags bits 8-9 pick one)
#define MR_UE 64  // (tile, face) entries per raster work unit (one wave, one entry per lane)
// ctr[CTR_ENTRIES64 .. +2) is a u64: list entries allocated by the per-view binning (k_bin_view)
// ctr[CTR_SENT]: fragments kept by the fused soft silhouette's raster (mr_soft_silhouette_forward)
// ctr[CTR_ZWALK]: tiles the K-deep raster walked near-to-far (its depth-ordered list walk)
// ctr[CTR_FLT]: non-zero once k_bwd_fused wrote a float remainder (a total component >= MR_FIX_MAX): the
// vertex-gradient gathers read the remainder rows only then (they are all zero otherwise)
enum { CTR_UNITS = 0, CTR_SLOTS = 1, CTR_COVERED = 2, CTR_SENT = 3, CTR_ENTRIES64 = 4, CTR_ZWALK = 6,
       CTR_FLT = 7, CTR_COUNT = 8 };

struct BinGeom {
  int TX, TY, T;
  int64_t list_cap;
  int64_t unit_cap;  // >= units the scan can emit: one per non-empty tile + list_cap / MR_UE
  int mfpb;          // max_faces_per_bin (0: none): a longer tile list takes the whole-view path
};
static BinGeom bin_geom(int H, int W, int64_t N, int64_t Ftot, int32_t mfpb) {
  BinGeom g;
  g.TX = ceil_div(W, MR_TS);
  g.TY = ceil_div(H, MR_TS);
  g.T = g.TX * g.TY;
  // Expected entries: ~(1 + 2*edge/8)^2 tiles per face + large faces; tiles whose list would
  // overflow take the exact full-view path (one unit scanning every face of the view).
  // max_faces_per_bin (if given) scales the reservation and caps each tile's list (PyTorch3D's per-bin cap).
  int64_t cap = 6 * Ftot + 2 * N * (int64_t)g.T + 65536;
  if (mfpb > 0) cap = (int64_t)mfpb * N * 16 + 65536;
  g.list_cap = cap < 0x40000000ll ? cap : 0x40000000ll;  // <= MR_CURSOR_OFF (k_bin_view); tiles past it take the exact path
  g.unit_cap = N * (int64_t)g.T + cap / MR_UE + 1;
  g.mfpb = mfpb > 0 ? mfpb : 0;
  return g;
}

static int num_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  }
  return cus;
}
// Workgroups (bands of tile rows) per view of the per-view binning: enough for the views to cover
// 1 / MR_BAND_CU_DIV of the CUs (1 view -> 64 bands, 16 views -> 4, 64 views -> 1 on 256 CUs), at
// most MR_BANDS_MAX and one tile row per band. The CUs left over stream the background beside the
// binning: banding 64 views 4 ways starved that share (fragment pass 421k -> 363k frames/s, render
// 240k -> 223k, profiles/r4f_bands_ab.txt). A pure function of the batch geometry: the backward's
// R/T reduction walks the same (view, band) ranges.
#ifndef MR_BAND_CU_DIV
#define MR_BAND_CU_DIV 4
#endif
static int bin_bands(int64_t N, const BinGeom& g) {
  int64_t b = (int64_t)num_cus() / ((N > 0 ? N : 1) * MR_BAND_CU_DIV);
  if (b > MR_BANDS_MAX) b = MR_BANDS_MAX;
  if (b > g.TY) b = g.TY;
  return b < 1 ? 1 : (int)b;
}
struct RasterWS {
  FaceRec* recs;
  int* ctr;    // (CTR_COUNT) units / slots emitted by the scan, covered pixels, entries (u64)
  int* cnt;    // (N*T) entries per tile; zeroed per call together with ctr and vtot (count -> scan path)
  int* vtot;   // (N) list entries per view (count -> scan path)
  uint32_t* rects;  // (2 * Ftot) per record: tile rectangle (k_bin_view path)
  int* start;  // (N*T) entry offset of each tile inside its view's region
  int* cur;    // (N*T) fill cursors
  int* vbase;  // (N) first list entry of each view (saturating)
  int* tdone;  // (N*T) per slot: units of a shared slot still to finish (count-down; the last writes)
  int* vslot;  // (2 N B) first slot and number of slots of each (view, band); B = 1 on the count -> scan path
  int* stile;  // (N*T) per slot: view * T + tile
  int4* units2;  // (unit_cap) the same units, heaviest first inside each XCD range (k_unit_order)
  int4* units; // (unit_cap) {view*T + tile, first list entry (-1: every face of the view), entries, slot | multi<<31}
  int* list;   // list_cap
  unsigned long long* tkey;  // (N*T*64) per-slot (z, face) keys of tiles shared by several units
  int* sface;  // (N*T*64) per slot, per tile pixel (row-major 8x8): winning face record or -1
  ShadeRec* srec;  // (F) per-face shading inputs (fused path; F = faces of the shared mesh)
  // (F, 27) u64 + (F, 27) f32: the fused backward's per-face gradient totals, cleared by the forward.
  // Fixed point (MR_FIX_SHIFT fractional bits, two's complement) summed with 64-bit integer atomics:
  // integer addition is associative, so the totals do not depend on the order the backward's waves
  // add their per-(record, tile) runs in — bitwise deterministic vertex gradients with one launch
  // fewer than a fixed-order reduction of stored rows (round 4). The f32 rows take the rare run
  // component of magnitude >= MR_FIX_MAX = 2^24 (float atomics; see mr_common.h).
  int* sorder;
  unsigned long long* gfix;
  float* gflt;
  float4* frec;    // (N*T*64) fused path: per slot pixel the winner's fragment (b0, b1, b2, signed dist)
  int* sgrp;       // (N*T*64) fused path: each slot's winners grouped by record (k_shade<1>, for the backward)
  uint8_t* sgpix;  // (N*T*64) fused path: the tile pixel of each grouped position
  ClipRec* crec;   // (2 * Ftot) barycentric conversion of near-plane sub-triangles (by record id)
  // banded per-view binning of one shared mesh (bands > 1): each (view, band)'s records, listed by
  // k_band_bucket (bcap = 2 Ftot / N: both triangles of every face of the view), and their counts
  // (cleared by the record launch)
  int* bcnt;
  int* blist;
  int64_t bcap;
  int nbcnt;       // N * bands (0: no lists)
  size_t bytes;
};
static RasterWS carve_raster_ws(void* base, int64_t N, int64_t Ftot, const BinGeom& g, int64_t Fshade = 0) {
  RasterWS w;
  Carver c(base);
  const size_t NT = (size_t)N * g.T, Fr = 2 * (size_t)(Ftot > 0 ? Ftot : 1), Fs = (size_t)Fshade;
  const size_t px = Fshade > 0 ? 64 * NT : 0;  // slot pixels of the fused path
  // face records: [0, Ftot) one per face instance, [Ftot, 2 Ftot) the second triangle of a face
  // split at the near plane (only written for such faces)
  w.recs = c.take<FaceRec>(Fr);
  w.ctr = c.take<int>(NT + (size_t)N + CTR_COUNT);  // 256-B aligned: the u64 entry counter at ctr + CTR_ENTRIES64
  w.cnt = w.ctr + CTR_COUNT;
  w.vtot = w.cnt + NT;
  w.rects = c.take<uint32_t>(Fr);
  w.start = c.take<int>(NT);
  w.cur = c.take<int>(NT);
  w.vbase = c.take<int>((size_t)N);
  w.tdone = c.take<int>(NT);
  w.vslot = c.take<int>(2 * MR_BANDS_MAX * (size_t)N);
  w.stile = c.take<int>(NT);
  w.units = c.take<int4>((size_t)g.unit_cap);
  w.units2 = c.take<int4>((size_t)g.unit_cap);  // the units in the raster's order (k_unit_order)
  w.list = c.take<int>((size_t)g.list_cap);
  w.tkey = c.take<unsigned long long>(64 * NT);
  w.sface = c.take<int>(64 * NT);
  w.srec = c.take<ShadeRec>(MR_SREC_SLOTS * Fs);  // MR_SREC_SLOTS slots of Fshade records (mr_render_reshade)
  w.sorder = c.take<int>(NT);  // the K-deep raster's slot order (k_slot_order)
  w.gfix = c.take<unsigned long long>(27 * Fs);
  w.gflt = c.take<float>(27 * Fs);
  w.frec = c.take<float4>(px);
  w.sgrp = c.take<int>(px);
  w.sgpix = c.take<uint8_t>(px);
  w.crec = c.take<ClipRec>(Fr);
  const int B = bin_bands(N, g);
  w.nbcnt = B > 1 ? (int)(N * B) : 0;
  w.bcap = B > 1 ? 2 * ((Ftot > 0 ? Ftot : 1) + N - 1) / N : 0;
  w.bcnt = c.take<int>((size_t)w.nbcnt);
  w.blist = c.take<int>((size_t)w.nbcnt * (size_t)w.bcap);
  w.bytes = c.off;
  return w;
}
// Bytes to clear from w.ctr before a forward: the counters and, on the count -> scan path, the
// per-tile counts and per-view totals.
static size_t zero_bytes(int64_t N, const BinGeom& g, bool view_path) {
  return sizeof(int) * (view_path ? (size_t)CTR_COUNT : (size_t)N * g.T + (size_t)N + CTR_COUNT);
}
