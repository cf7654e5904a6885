// rt_calls.hip — the calls beside the frame, over the C ABI (include/uob_rt.h): ray queries (rt_trace_rays, rt_ray_query.hip),
// shade calls (rt_shade_points, rt_shade.hip), radiance calls (rt_radiance_rays, rt_radiance.hip), AOV passes
// (rt_render_aov, rt_aov.hip), filter calls (rt_filter_plane, rt_filter.hip; rt_filter_plane_variance, rt_filter_variance.hip), accumulate calls (rt_accumulate_plane,
// rt_accumulate.hip) and motion calls with their snapshot (rt_motion_planes, rt_motion.hip).  Each family has an enqueue on the caller's stream (the *_device entry), a blocking entry for
// host arrays that stages them through the family's device buffer, and a stats export.  What the families share is written
// once: the steps around a call (call_prepare / reader_begin / call_end), the blocking entry (run_blocking) and the stats
// reader (read_stats).  Which operation waits for which is DESIGN.md 4.9 (rt_host.h wait_scene_readers, wait_aov, wait_scene).
#include <cmath>
#include <cstring>

#include "rt_host.h"

using namespace uobrt;

// Make sure the buffer holds `bytes`.  Regrowing frees the old buffer first: hipFree synchronises with the device, so
// whatever still uses the old buffer has finished before it goes.
int uobrt::ensure_bytes(DevBuffer* b, size_t bytes) {
  if (bytes <= b->bytes) return RT_OK;
  b->reset();
  return b->alloc(bytes) == hipSuccess ? RT_OK : alloc_failed();
}

// ---- around a call -------------------------------------------------------------------------------------------------------
// Before anything of a call is enqueued: the device, and the family's event and counters on first use
static int call_prepare(rt_ctx* c, SideCall* k, int stats_words) {
  HIP_TRY(hipSetDevice(c->device));
  if (!k->ev) HIP_TRY(k->ev.create(hipEventDisableTiming));
  if (!k->d_stats && k->d_stats.alloc((size_t)stats_words) != hipSuccess) return alloc_failed();
  return RT_OK;
}

// A reader of the scene on stream s: prepared, behind the latest update and the latest call of every reader family,
// counters zeroed
static int reader_begin(rt_ctx* c, SideCall* k, int stats_words, hipStream_t s) {
  const size_t stats_bytes = (size_t)stats_words * sizeof(unsigned long long);
  const int rc = call_prepare(c, k, stats_words);
  if (rc != RT_OK) return rc;
  HIP_TRY(wait_scene(c, s));
  if (wait_scene_readers(c, s) != RT_OK) return RT_E_DEVICE;
  HIP_TRY(hipMemsetAsync(k->d_stats, 0, stats_bytes, s));
  return RT_OK;
}

// Behind the call's kernels: launch errors, the family's event, and what its stats export reports besides the counters
static int call_end(rt_ctx* c, SideCall* k, hipStream_t s) {
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(k->ev, s));
  k->pending = true;
  k->tiles = c->d_verts_m ? mesh_tiles(c->n) : 0;
  return RT_OK;
}

// ---- blocking entries -------------------------------------------------------------------------------------------------------
// One host array of a blocking entry: uploaded before the call (in) or downloaded after it; host == nullptr: not asked for,
// takes no room.  run_blocking fills dev, the array's place in the family's staging buffer, in the order of the list.
struct IoSlot {
  void* host;
  size_t bytes;
  bool in;
  char* dev;
};

// The blocking entry of a family, c a single-device context: lay the slots out, make room, upload the inputs on c->stream,
// enqueue (the callable sees the slots' dev pointers), download the outputs, synchronise
template <class Enqueue>
static int run_blocking(rt_ctx* c, SideCall* k, IoSlot* slot, int nslot, Enqueue enqueue) {
  HIP_TRY(hipSetDevice(c->device));
  size_t bytes = 0;
  for (int i = 0; i < nslot; ++i) if (slot[i].host) bytes += slot[i].bytes;
  int rc = ensure_bytes(&k->io, bytes);          // (only this blocking entry uses the buffer: nothing can still be reading it)
  if (rc != RT_OK) return rc;
  char* d = k->io.p;
  for (int i = 0; i < nslot; ++i) { slot[i].dev = slot[i].host ? d : nullptr; if (slot[i].host) d += slot[i].bytes; }
  for (int i = 0; i < nslot; ++i)
    if (slot[i].host && slot[i].in) HIP_TRY(hipMemcpyAsync(slot[i].dev, slot[i].host, slot[i].bytes, hipMemcpyHostToDevice, c->stream));
  rc = enqueue();
  if (rc != RT_OK) { hipStreamSynchronize(c->stream); return rc; }
  for (int i = 0; i < nslot; ++i)
    if (slot[i].host && !slot[i].in) HIP_TRY(hipMemcpyAsync(slot[i].host, slot[i].dev, slot[i].bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RT_OK;
}

// The domain of global_id: beyond 2^24 the reference's float products lose the id
static int check_seeds(const int32_t* seeds, int64_t n, const char* fn) {
  if (seeds)
    for (int64_t k = 0; k < n; ++k)
      if (seeds[k] < 0 || seeds[k] > (1 << 24)) {
        set_error("%s: seeds[%lld] = %d outside [0, 2^24]", fn, (long long)k, seeds[k]); return RT_E_INVALID;
      }
  return RT_OK;
}

// The counters of a family's latest call, once it has finished; tile_slot: where the tile count goes (-1: nowhere)
static int read_stats(rt_ctx* c, SideCall rt_ctx::*family, int tile_slot, uint64_t out[8]) {
  if (!c || !out) { set_error("NULL argument"); return RT_E_INVALID; }
  memset(out, 0, 8 * sizeof(uint64_t));
  c = lead_ctx(c);
  const SideCall& k = c->*family;
  if (!k.pending) return RT_OK;
  DeviceGuard guard;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(k.ev));
  HIP_TRY(hipMemcpy(out, k.d_stats, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (tile_slot >= 0) out[tile_slot] = (uint64_t)k.tiles;
  return RT_OK;
}

// ---- ray queries (rt_trace_rays / rt_trace_rays_device, rt_ray_query.hip) ---------------------------------------------
static int check_query_args(const rt_ctx* c, int32_t what, const void* rays6, const void* radius_sq, int64_t nray,
                            const void* out_tri, const char* fn) {
  if (!c || !rays6 || !out_tri) { set_error("%s: NULL argument", fn); return RT_E_INVALID; }
  if (what != RT_TRACE_IN_SHADOW && what != RT_TRACE_CLOSEST_HIT) { set_error("%s: unknown mode %d", fn, what); return RT_E_INVALID; }
  if (nray < 0 || nray > (int64_t(1) << 36)) { set_error("%s: nray = %lld outside [0, 2^36]", fn, (long long)nray); return RT_E_INVALID; }
  if (what == RT_TRACE_IN_SHADOW && !radius_sq) { set_error("%s: radius_sq missing", fn); return RT_E_INVALID; }
  return RT_OK;
}

// One query of a single-device context on stream s (device buffers of c->device); nray > 0, arguments checked
static int enqueue_query(rt_ctx* c, int32_t what, const float* d_rays, const float* d_r2, long nray, int* d_tri, float* d_out10,
                         hipStream_t s) {
  const bool tiled = c->d_verts_m != nullptr;
  const bool records = !tiled && generic_needs_records(c->n);
  const int rc = reader_begin(c, &c->query, query_stats_words(), s);
  if (rc != RT_OK) return rc;
  if (records && !c->d_qrecords && c->d_qrecords.alloc((size_t)c->cap * kRecordsPerTriangle) != hipSuccess) return alloc_failed();
  const float zero3[3] = {0.f, 0.f, 0.f};
  FrameParams P;
  scene_params(c, zero3, tiled, &P);
  P.records = records ? c->d_qrecords : nullptr;
  if (records) launch_stage_records(P, s);
  launch_query(P, tiled, what, d_rays, d_r2, nray, d_tri, what == RT_TRACE_CLOSEST_HIT ? d_out10 : nullptr, c->query.d_stats, c->cus, s);
  return call_end(c, &c->query, s);
}

// ---- shade calls (rt_shade_points / rt_shade_points_device, rt_shade.hip) -----------------------------------------------
// The arguments of a shade or radiance call (`count` names n in the message); checked before the context is looked at, like
// the queries' arguments
static int check_lit_args(const rt_ctx* c, const void* in6, int64_t n, const float* light, const void* out, const char* fn,
                          const char* count) {
  if (!c || !in6 || !light || !out) { set_error("%s: NULL argument", fn); return RT_E_INVALID; }
  if (n < 0 || n > (int64_t(1) << 31)) { set_error("%s: %s = %lld outside [0, 2^31]", fn, count, (long long)n); return RT_E_INVALID; }
  return RT_OK;
}

// One shade call of a single-device context on stream s (device buffers of c->device); npoints > 0, arguments checked
static int enqueue_shade(rt_ctx* c, const float* d_points6, const int* d_seeds, long npoints, const float light[3], float* d_light,
                         int* d_cnt, hipStream_t s) {
  const bool tiled = c->d_verts_m != nullptr;
  const int rc = reader_begin(c, &c->shade, shade_stats_words(), s);
  if (rc != RT_OK) return rc;
  FrameParams P;
  scene_params(c, light, tiled, &P);
  launch_shade(P, tiled, d_points6, d_seeds, npoints, d_light, d_cnt, c->shade.d_stats, c->cus, s);
  return call_end(c, &c->shade, s);
}

// ---- radiance calls (rt_radiance_rays / rt_radiance_rays_device, rt_radiance.hip) --------------------------------------
// One radiance call of a single-device context on stream s (device buffers of c->device); nray > 0, arguments checked
static int enqueue_radiance(rt_ctx* c, const float* d_rays6, const int* d_seeds, long nray, const float light[3], float* d_rgba4,
                            int* d_prim, hipStream_t s) {
  const bool tiled = c->d_verts_m != nullptr;
  int rc = reader_begin(c, &c->rad, radiance_stats_words(), s);
  if (rc != RT_OK) return rc;
  rc = ensure_bytes(&c->rrec, radiance_record_bytes(nray));   // (a larger call than any before: hipFree waits for the call still using the old one)
  if (rc != RT_OK) return rc;
  FrameParams P;
  scene_params(c, light, tiled, &P);
  launch_radiance(P, tiled, d_rays6, d_seeds, nray, (float4*)d_rgba4, d_prim, (float4*)c->rrec.p, c->rad.d_stats, c->cus, s);
  return call_end(c, &c->rad, s);
}

// ---- AOV passes (rt_render_aov / rt_render_aov_device, rt_aov.hip) ----------------------------------------------------
// Checked before the context is looked at, so that the struct's own errors are reported for any context
static int check_aov_args(const rt_ctx* c, const float* rot, const float* cam, const rt_aov_buffers* b, const char* fn) {
  if (!b) { set_error("%s: the buffers struct is NULL", fn); return RT_E_INVALID; }
  if (!b->prim && !b->depth && !b->position4 && !b->normal4 && !b->albedo4 && !b->direction4) {
    set_error("%s: no plane requested (every pointer of the buffers struct is NULL)", fn); return RT_E_INVALID;
  }
  if (!c) { set_error("%s: ctx is NULL", fn); return RT_E_INVALID; }
  if (!rot || !cam) { set_error("%s: rot / cam is NULL", fn); return RT_E_INVALID; }
  return RT_OK;
}

// One pass of a single-device context on stream s into device planes of c->device.  `whole`: c is devices[0] of a
// multi-device context and renders every row of the frame, not only its own bands.
static int enqueue_aov(rt_ctx* c, const float rot[12], const float cam[3], float focal, int32_t sample, const AovPlanes& A,
                       bool whole, hipStream_t s) {
  const int aa = c->cfg.aa_x * c->cfg.aa_y;
  if (sample != RT_AOV_ALL_SAMPLES && (sample < 0 || sample >= aa)) {
    set_error("rt_render_aov: sample = %d outside [0, %d) and not RT_AOV_ALL_SAMPLES", sample, aa); return RT_E_INVALID;
  }
  for (int k = 0; k < 3; ++k)
    if (!(fabsf(cam[k]) <= kMaxCoordinate)) { set_error("camera coordinates must be finite and <= 2^16"); return RT_E_INVALID; }
  if (!(fabsf(focal) <= 1.0e9f)) { set_error("focal length must be finite and <= 1e9"); return RT_E_INVALID; }
  for (int k = 0; k < 12; ++k)
    if (!(fabsf(rot[k]) <= 4.0f)) { set_error("rotation matrix entries must be finite and <= 4"); return RT_E_INVALID; }
  const int rows = whole ? c->cfg.height : c->owned_rows;
  if (rows == 0) return RT_OK;
  const size_t stats_bytes = (size_t)aov_stats_words() * sizeof(unsigned long long);
  const int rc = call_prepare(c, &c->aov, aov_stats_words());
  if (rc != RT_OK) return rc;
  const float zero3[3] = {0.f, 0.f, 0.f};
  FrameParams P;
  fill_params(c, rot, cam, zero3, focal, &P);
  if (whole) {                                 // all rows of the frame in image order
    P.band_rows = c->cfg.height; P.band_index = 0; P.band_count = 1; P.owned_rows = rows;
    P.band_rows_magic = div_magic_for(P.band_rows);
  }
  const bool tiled = c->d_verts_m != nullptr;
  const bool bins = tiled && c->d_screen_masks != nullptr && c->d_records != nullptr && !(c->tune.mask_debug & 1);
  if (!bins) P.screen_masks = nullptr;
  // one frame-like operation of a context at a time: the records and the screen masks are the frames'
  if (c->timed && s != c->last_stream) HIP_TRY(hipStreamWaitEvent(s, c->ev1, 0));
  HIP_TRY(wait_aov(c, s));
  HIP_TRY(wait_scene(c, s));
  HIP_TRY(hipMemsetAsync(c->aov.d_stats, 0, stats_bytes, s));
  if (tiled) {
    use_tiled_scene(c, &P);
    if (bins) { launch_stage_records(P, s); launch_bin_primary(P, s); }   // the masks are built from this view's records
  } else if (generic_needs_records(c->n)) {
    launch_stage_records(P, s);
  }
  launch_aov(P, tiled, A, sample, c->aov.d_stats, c->cus, s);
  c->aov_stream = s;                           // (wait_aov: a later operation on this stream is behind the pass anyway)
  return call_end(c, &c->aov, s);
}

// ---- filter calls (rt_filter_plane / rt_filter_plane_device, rt_filter.hip) ---------------------------------------------
// One filter call of a single-device context on stream s (device planes of c->device); arguments checked.  Not a reader of
// the scene: it waits for the filter call before it, whose scratch it takes over, and for nothing else.
static int enqueue_filter(rt_ctx* c, const rt_filter_params& p, const float* d_value, const float4* d_pos, const float4* d_nrm,
                          float* d_out, hipStream_t s) {
  const size_t count = (size_t)p.width * p.height;
  const int words = filter_stats_words();
  int rc = call_prepare(c, &c->filter, words);
  if (rc != RT_OK) return rc;
  rc = ensure_bytes(&c->filter_guides, count * 32);   // (a larger call than any before: hipFree waits for the call still using the old one)
  if (rc == RT_OK) rc = ensure_bytes(&c->filter_planes, count * 8);
  if (rc != RT_OK) return rc;
  if (c->filter.pending) HIP_TRY(hipStreamWaitEvent(s, c->filter.ev, 0));
  HIP_TRY(hipMemsetAsync(c->filter.d_stats, 0, (size_t)words * sizeof(unsigned long long), s));
  float4* rec = (float4*)c->filter_guides.p;
  float* plane[2] = {(float*)c->filter_planes.p, (float*)c->filter_planes.p + count};
  launch_filter_pack(d_pos, d_nrm, (long)count, p.passes, rec, c->filter.d_stats, s);
  // no pass reads what it writes: the passes alternate between the two planes and the last one writes d_out — through a
  // plane and a copy when it is also the first and the call is in place
  const bool bounce = p.passes == 1 && d_out == d_value;
  const float* src = d_value;
  for (int i = 0; i < p.passes; ++i) {
    float* dst = (i == p.passes - 1 && !bounce) ? d_out : plane[i & 1];
    launch_filter_pass(p, i, c->tune.filter_form, rec, src, dst, c->filter.d_stats, s);
    src = dst;
  }
  launch_filter_counters(c->filter.d_stats, s);
  if (bounce) HIP_TRY(hipMemcpyAsync(d_out, src, count * sizeof(float), hipMemcpyDeviceToDevice, s));
  return call_end(c, &c->filter, s);
}

// One variance-guided filter call (rt_filter_plane_variance*, rt_filter_variance.hip) of a single-device context on stream s;
// arguments checked, d_out_var may be NULL.  A call of the filter family: the plain calls' event, counters, guides and value
// planes, and 12 bytes per pixel of its own (two variance planes, the thresholds).
static int enqueue_filter_variance(rt_ctx* c, const rt_filter_variance_params& vp, const float* d_value, const float* d_var,
                                   const float4* d_pos, const float4* d_nrm, float* d_out, float* d_out_var, hipStream_t s) {
  const rt_filter_params& p = vp.base;
  const size_t count = (size_t)p.width * p.height;
  const int words = filter_stats_words();
  int rc = call_prepare(c, &c->filter, words);
  if (rc != RT_OK) return rc;
  rc = ensure_bytes(&c->filter_guides, count * 32);   // (a larger call than any before: hipFree waits for the call still using the old one)
  if (rc == RT_OK) rc = ensure_bytes(&c->filter_planes, count * 8);
  if (rc == RT_OK) rc = ensure_bytes(&c->filter_variance, count * 12);
  if (rc != RT_OK) return rc;
  if (c->filter.pending) HIP_TRY(hipStreamWaitEvent(s, c->filter.ev, 0));
  HIP_TRY(hipMemsetAsync(c->filter.d_stats, 0, (size_t)words * sizeof(unsigned long long), s));
  float4* rec = (float4*)c->filter_guides.p;
  float* plane[2] = {(float*)c->filter_planes.p, (float*)c->filter_planes.p + count};
  float* vplane[2] = {(float*)c->filter_variance.p, (float*)c->filter_variance.p + count};
  float* T = (float*)c->filter_variance.p + 2 * count;
  launch_filter_pack(d_pos, d_nrm, (long)count, p.passes, rec, c->filter.d_stats, s);
  // no pass reads what it writes: the passes alternate between the scratch planes and the last one writes the outputs —
  // through a scratch plane and a copy where it is also the first and that plane is filtered in place.  Without
  // d_out_var the last pass leaves the variance in the scratch
  const bool bounce = p.passes == 1 && d_out == d_value, vbounce = p.passes == 1 && d_out_var == d_var;
  const float *src = d_value, *vsrc = d_var;
  for (int i = 0; i < p.passes; ++i) {
    const bool last = i == p.passes - 1;
    float* dst = (last && !bounce) ? d_out : plane[i & 1];
    float* vdst = (last && !vbounce && d_out_var) ? d_out_var : vplane[i & 1];
    launch_filter_variance_threshold(vp, rec, vsrc, T, s);
    launch_filter_variance_pass(vp, i, c->tune.filter_form, rec, T, src, vsrc, dst, vdst, c->filter.d_stats, s);
    src = dst;
    vsrc = vdst;
  }
  launch_filter_variance_counters(c->filter.d_stats, s);
  if (bounce) HIP_TRY(hipMemcpyAsync(d_out, src, count * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (vbounce) HIP_TRY(hipMemcpyAsync(d_out_var, vsrc, count * sizeof(float), hipMemcpyDeviceToDevice, s));
  return call_end(c, &c->filter, s);
}

// ---- accumulate calls (rt_accumulate_plane / rt_accumulate_plane_device, rt_accumulate.hip) ---------------------------
// One accumulate call of a single-device context on stream s (device planes of c->device); arguments checked.  Not a reader
// of the scene: it waits for the accumulate call before it, whose counters it takes over, and for nothing else.
static int enqueue_accumulate(rt_ctx* c, const rt_accumulate_params& p, const float* d_value, const float4* d_pos, const float4* d_nrm,
                              const int* d_prim, const float4* d_rpos, const float4* d_rnrm, const float4* d_prev, float4* d_next,
                              float* d_mean, float* d_var, hipStream_t s) {
  const int words = accumulate_stats_words();
  const int rc = call_prepare(c, &c->accum, words);
  if (rc != RT_OK) return rc;
  if (c->accum.pending) HIP_TRY(hipStreamWaitEvent(s, c->accum.ev, 0));
  HIP_TRY(hipMemsetAsync(c->accum.d_stats, 0, (size_t)words * sizeof(unsigned long long), s));
  launch_accumulate(p, d_value, d_pos, d_nrm, d_prim, d_rpos, d_rnrm, d_prev, d_next, d_mean, d_var, c->accum.d_stats, s);
  return call_end(c, &c->accum, s);
}

// The two entries for device planes and the two for host arrays; reproj: the entry takes the reprojection planes (fn names it)
static int accumulate_device_entry(rt_ctx* c, const rt_accumulate_params* p, const void* d_value, const void* d_position4,
                                   const void* d_normal4, const void* d_prim, const void* d_rpos, const void* d_rnrm, const void* d_prev,
                                   void* d_next, void* d_out_mean, void* d_out_variance, void* hip_stream, const char* fn) {
  if (!c) { set_error("%s: ctx is NULL", fn); return RT_E_INVALID; }
  int rc = accumulate_check(p, d_value, d_position4, d_normal4, d_prev, d_next, fn);
  if (rc == RT_OK) rc = accumulate_reproj_check(d_rpos, d_rnrm, fn);
  if (rc != RT_OK) return rc;
  if ((((uintptr_t)d_position4 | (uintptr_t)d_normal4 | (uintptr_t)d_prev | (uintptr_t)d_next) & 15) != 0) {
    set_error("%s: d_position4 / d_normal4 / d_prev / d_next is not 16-byte aligned", fn); return RT_E_INVALID;
  }
  if ((((uintptr_t)d_rpos | (uintptr_t)d_rnrm) & 15) != 0) {
    set_error("%s: d_reproj_position4 / d_reproj_normal4 is not 16-byte aligned", fn); return RT_E_INVALID;
  }
  DeviceGuard guard;
  return enqueue_accumulate(lead_ctx(c), *p, (const float*)d_value, (const float4*)d_position4, (const float4*)d_normal4,
                            (const int*)d_prim, (const float4*)d_rpos, (const float4*)d_rnrm, (const float4*)d_prev, (float4*)d_next,
                            (float*)d_out_mean, (float*)d_out_variance, (hipStream_t)hip_stream);
}

static int accumulate_blocking_entry(rt_ctx* c, const rt_accumulate_params* p, const float* value, const float* position4,
                                     const float* normal4, const int32_t* prim, const float* rpos, const float* rnrm,
                                     const rt_history_texel* prev, rt_history_texel* next, float* out_mean, float* out_variance,
                                     const char* fn) {
  if (!c) { set_error("%s: ctx is NULL", fn); return RT_E_INVALID; }
  int rc = accumulate_check(p, value, position4, normal4, prev, next, fn);
  if (rc == RT_OK) rc = accumulate_reproj_check(rpos, rnrm, fn);
  if (rc != RT_OK) return rc;
  c = lead_ctx(c);
  DeviceGuard guard;
  const size_t n = (size_t)p->width * p->height;
  // (what the kernel loads and stores as float4 first: the start of the staging buffer is aligned for that, and every one
  // of these is a multiple of 16 bytes long)
  IoSlot io[10] = {{(void*)position4, n * 16, true}, {(void*)normal4, n * 16, true}, {(void*)rpos, n * 16, true}, {(void*)rnrm, n * 16, true},
                   {(void*)prev, n * 48, true},      {next, n * 48, false},          {(void*)value, n * 4, true}, {(void*)prim, n * 4, true},
                   {out_mean, n * 4, false},         {out_variance, n * 4, false}};
  return run_blocking(c, &c->accum, io, 10, [&] {
    return enqueue_accumulate(c, *p, (const float*)io[6].dev, (const float4*)io[0].dev, (const float4*)io[1].dev, (const int*)io[7].dev,
                              (const float4*)io[2].dev, (const float4*)io[3].dev, (const float4*)io[4].dev, (float4*)io[5].dev,
                              (float*)io[8].dev, (float*)io[9].dev, c->stream);
  });
}

// ---- motion calls and their snapshot (rt_motion_snapshot / rt_motion_planes*, rt_motion.hip) ------------------------------
// A snapshot or a motion call on stream s: prepared, behind the latest edit and the family's previous call.  Readers of the
// scene (wait_scene_readers lists the family, so edits wait for them); frames and AOV passes neither wait nor are waited for.
static int motion_begin(rt_ctx* c, hipStream_t s) {
  const bool first = !c->motion.d_stats;
  const int rc = call_prepare(c, &c->motion, motion_stats_words());
  if (rc != RT_OK) return rc;
  HIP_TRY(wait_scene(c, s));
  if (c->motion.pending) HIP_TRY(hipStreamWaitEvent(s, c->motion.ev, 0));
  // (a snapshot writes no counters: before the first motion call the export reads zeros)
  if (first) HIP_TRY(hipMemsetAsync(c->motion.d_stats, 0, (size_t)motion_stats_words() * sizeof(unsigned long long), s));
  return RT_OK;
}

// The context that answers a motion call holds a snapshot of its current triangle count
static int check_snapshot(const rt_ctx* c, const char* fn) {
  if (!c->motion_taken) { set_error("%s: the context holds no snapshot (rt_motion_snapshot)", fn); return RT_E_INVALID; }
  if (c->motion_n != c->n) {
    set_error("%s: the snapshot holds %d triangles, the scene %d (take a new rt_motion_snapshot)", fn, c->motion_n, c->n); return RT_E_INVALID;
  }
  return RT_OK;
}

// One motion call of a single-device context on stream s (device planes of c->device); count > 0, arguments checked
static int enqueue_motion(rt_ctx* c, const int* d_prim, const float4* d_pos, const float4* d_nrm, long count, float4* d_out_pos,
                          float4* d_out_nrm, hipStream_t s) {
  const int words = motion_stats_words();
  const int rc = motion_begin(c, s);
  if (rc != RT_OK) return rc;
  HIP_TRY(hipMemsetAsync(c->motion.d_stats, 0, (size_t)words * sizeof(unsigned long long), s));
  launch_motion(c->d_verts, c->motion_verts, c->motion_normals, c->n, d_prim, d_pos, d_nrm, count, d_out_pos, d_out_nrm,
                c->tune.motion_blocks_x, c->motion.d_stats, s);
  return call_end(c, &c->motion, s);
}

extern "C" {

int rt_accumulate_plane_device(rt_ctx* c, const rt_accumulate_params* p, const void* d_value, const void* d_position4,
                               const void* d_normal4, const void* d_prim, const void* d_prev, void* d_next, void* d_out_mean,
                               void* d_out_variance, void* hip_stream) {
  return accumulate_device_entry(c, p, d_value, d_position4, d_normal4, d_prim, nullptr, nullptr, d_prev, d_next, d_out_mean,
                                 d_out_variance, hip_stream, "rt_accumulate_plane_device");
}

int rt_accumulate_plane(rt_ctx* c, const rt_accumulate_params* p, const float* value, const float* position4, const float* normal4,
                        const int32_t* prim, const rt_history_texel* prev, rt_history_texel* next, float* out_mean,
                        float* out_variance) {
  return accumulate_blocking_entry(c, p, value, position4, normal4, prim, nullptr, nullptr, prev, next, out_mean, out_variance,
                                   "rt_accumulate_plane");
}

int rt_accumulate_plane_moving_device(rt_ctx* c, const rt_accumulate_params* p, const void* d_value, const void* d_position4,
                                      const void* d_normal4, const void* d_prim, const void* d_reproj_position4,
                                      const void* d_reproj_normal4, const void* d_prev, void* d_next, void* d_out_mean,
                                      void* d_out_variance, void* hip_stream) {
  return accumulate_device_entry(c, p, d_value, d_position4, d_normal4, d_prim, d_reproj_position4, d_reproj_normal4, d_prev, d_next,
                                 d_out_mean, d_out_variance, hip_stream, "rt_accumulate_plane_moving_device");
}

int rt_accumulate_plane_moving(rt_ctx* c, const rt_accumulate_params* p, const float* value, const float* position4,
                               const float* normal4, const int32_t* prim, const float* reproj_position4, const float* reproj_normal4,
                               const rt_history_texel* prev, rt_history_texel* next, float* out_mean, float* out_variance) {
  return accumulate_blocking_entry(c, p, value, position4, normal4, prim, reproj_position4, reproj_normal4, prev, next, out_mean,
                                   out_variance, "rt_accumulate_plane_moving");
}

int rt_motion_snapshot(rt_ctx* c, void* hip_stream) {
  if (!c) { set_error("rt_motion_snapshot: ctx is NULL"); return RT_E_INVALID; }
  c = lead_ctx(c);
  DeviceGuard guard;
  const hipStream_t s = (hipStream_t)hip_stream;
  const int rc = motion_begin(c, s);
  if (rc != RT_OK) return rc;
  const size_t n = (size_t)c->n;
  // (a larger scene than any snapshot before: hipFree waits for the motion call still reading the old buffers)
  if (3 * n * sizeof(float4) > c->motion_verts.bytes || !c->motion_verts) {
    c->motion_taken = false;
    if (c->motion_verts.alloc(3 * n) != hipSuccess || c->motion_normals.alloc(n) != hipSuccess) {
      c->motion_verts.reset(); c->motion_normals.reset();
      return alloc_failed();
    }
  }
  if (n) {
    HIP_TRY(hipMemcpyAsync(c->motion_verts, c->d_verts, 3 * n * sizeof(float4), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->motion_normals, c->d_normals, n * sizeof(float4), hipMemcpyDeviceToDevice, s));
  }
  c->motion_n = c->n;
  c->motion_taken = true;
  return call_end(c, &c->motion, s);
}

int rt_motion_release(rt_ctx* c) {
  if (!c) { set_error("rt_motion_release: ctx is NULL"); return RT_E_INVALID; }
  c = lead_ctx(c);
  DeviceGuard guard;
  HIP_TRY(hipSetDevice(c->device));
  if (c->motion.pending) HIP_TRY(hipEventSynchronize(c->motion.ev));   // (no snapshot copy or motion call still uses the buffers)
  c->motion_verts.reset();
  c->motion_normals.reset();
  c->motion_n = 0;
  c->motion_taken = false;
  return RT_OK;
}

int rt_debug_motion_info(rt_ctx* c, int32_t* snapshot_triangles) {
  if (!c || !snapshot_triangles) { set_error("rt_debug_motion_info: NULL argument"); return RT_E_INVALID; }
  c = lead_ctx(c);
  *snapshot_triangles = c->motion_taken ? c->motion_n : 0;
  return RT_OK;
}

int rt_motion_planes_device(rt_ctx* c, const void* d_prim, const void* d_position4, const void* d_normal4, int64_t count,
                            void* d_out_prev_position4, void* d_out_prev_normal4, void* hip_stream) {
  if (!c) { set_error("rt_motion_planes_device: ctx is NULL"); return RT_E_INVALID; }
  int rc = motion_check(d_prim, d_position4, d_normal4, count, d_out_prev_position4, d_out_prev_normal4, "rt_motion_planes_device");
  if (rc != RT_OK) return rc;
  if ((((uintptr_t)d_position4 | (uintptr_t)d_normal4 | (uintptr_t)d_out_prev_position4 | (uintptr_t)d_out_prev_normal4) & 15) != 0) {
    set_error("rt_motion_planes_device: d_position4 / d_normal4 / d_out_prev_position4 / d_out_prev_normal4 is not 16-byte aligned");
    return RT_E_INVALID;
  }
  c = lead_ctx(c);
  rc = check_snapshot(c, "rt_motion_planes_device");
  if (rc != RT_OK || count == 0) return rc;
  DeviceGuard guard;
  return enqueue_motion(c, (const int*)d_prim, (const float4*)d_position4, (const float4*)d_normal4, (long)count,
                        (float4*)d_out_prev_position4, (float4*)d_out_prev_normal4, (hipStream_t)hip_stream);
}

int rt_motion_planes(rt_ctx* c, const int32_t* prim, const float* position4, const float* normal4, int64_t count,
                     float* out_prev_position4, float* out_prev_normal4) {
  if (!c) { set_error("rt_motion_planes: ctx is NULL"); return RT_E_INVALID; }
  int rc = motion_check(prim, position4, normal4, count, out_prev_position4, out_prev_normal4, "rt_motion_planes");
  if (rc != RT_OK) return rc;
  c = lead_ctx(c);
  rc = check_snapshot(c, "rt_motion_planes");
  if (rc != RT_OK || count == 0) return rc;
  DeviceGuard guard;
  const size_t n = (size_t)count;
  // (the float4 planes first: the start of the staging buffer is aligned for them)
  IoSlot io[5] = {{(void*)position4, n * 16, true}, {(void*)normal4, n * 16, true}, {out_prev_position4, n * 16, false},
                  {out_prev_normal4, n * 16, false}, {(void*)prim, n * 4, true}};
  return run_blocking(c, &c->motion, io, 5, [&] {
    return enqueue_motion(c, (const int*)io[4].dev, (const float4*)io[0].dev, (const float4*)io[1].dev, (long)count, (float4*)io[2].dev,
                          (float4*)io[3].dev, c->stream);
  });
}

int rt_debug_motion_stats(rt_ctx* c, uint64_t out[8]) {
  const int rc = read_stats(c, &rt_ctx::motion, -1, out);
  if (rc == RT_OK) out[6] = out[7] = 0;
  return rc;
}

int rt_debug_accumulate_stats(rt_ctx* c, uint64_t out[8]) {
  const int rc = read_stats(c, &rt_ctx::accum, -1, out);
  if (rc == RT_OK) out[5] = out[6] = out[7] = 0;
  return rc;
}

int rt_filter_plane_device(rt_ctx* c, const rt_filter_params* p, const void* d_value, const void* d_position4, const void* d_normal4,
                           void* d_out, void* hip_stream) {
  if (!c) { set_error("rt_filter_plane_device: ctx is NULL"); return RT_E_INVALID; }
  const int rc = filter_check(p, d_value, d_position4, d_normal4, d_out, "rt_filter_plane_device");
  if (rc != RT_OK) return rc;
  if ((((uintptr_t)d_position4 | (uintptr_t)d_normal4) & 15) != 0) {
    set_error("rt_filter_plane_device: d_position4 / d_normal4 is not 16-byte aligned"); return RT_E_INVALID;
  }
  DeviceGuard guard;
  return enqueue_filter(lead_ctx(c), *p, (const float*)d_value, (const float4*)d_position4, (const float4*)d_normal4, (float*)d_out,
                        (hipStream_t)hip_stream);
}

int rt_filter_plane(rt_ctx* c, const rt_filter_params* p, const float* value, const float* position4, const float* normal4, float* out) {
  if (!c) { set_error("rt_filter_plane: ctx is NULL"); return RT_E_INVALID; }
  const int rc = filter_check(p, value, position4, normal4, out, "rt_filter_plane");
  if (rc != RT_OK) return rc;
  c = lead_ctx(c);
  DeviceGuard guard;
  const size_t n = (size_t)p->width * p->height;
  // (the guides first: the kernels load them as float4, and the start of the staging buffer is aligned for that)
  IoSlot io[4] = {{(void*)position4, n * 16, true}, {(void*)normal4, n * 16, true}, {(void*)value, n * 4, true}, {out, n * 4, false}};
  return run_blocking(c, &c->filter, io, 4, [&] {
    return enqueue_filter(c, *p, (const float*)io[2].dev, (const float4*)io[0].dev, (const float4*)io[1].dev, (float*)io[3].dev, c->stream);
  });
}

int rt_debug_filter_stats(rt_ctx* c, uint64_t out[8]) {
  const int rc = read_stats(c, &rt_ctx::filter, -1, out);
  if (rc == RT_OK) out[6] = out[7] = 0;             // (out[5]: written by a variance call only, 0 after a plain one)
  return rc;
}

int rt_filter_plane_variance_device(rt_ctx* c, const rt_filter_variance_params* p, const void* d_value, const void* d_variance,
                                    const void* d_position4, const void* d_normal4, void* d_out_value, void* d_out_variance,
                                    void* hip_stream) {
  const char* fn = "rt_filter_plane_variance_device";
  if (!c) { set_error("%s: ctx is NULL", fn); return RT_E_INVALID; }
  const int rc = filter_variance_check(p, d_value, d_variance, d_position4, d_normal4, d_out_value, fn);
  if (rc != RT_OK) return rc;
  if ((((uintptr_t)d_position4 | (uintptr_t)d_normal4) & 15) != 0) {
    set_error("%s: d_position4 / d_normal4 is not 16-byte aligned", fn); return RT_E_INVALID;
  }
  DeviceGuard guard;
  return enqueue_filter_variance(lead_ctx(c), *p, (const float*)d_value, (const float*)d_variance, (const float4*)d_position4,
                                 (const float4*)d_normal4, (float*)d_out_value, (float*)d_out_variance, (hipStream_t)hip_stream);
}

int rt_filter_plane_variance(rt_ctx* c, const rt_filter_variance_params* p, const float* value, const float* variance,
                             const float* position4, const float* normal4, float* out_value, float* out_variance) {
  const char* fn = "rt_filter_plane_variance";
  if (!c) { set_error("%s: ctx is NULL", fn); return RT_E_INVALID; }
  const int rc = filter_variance_check(p, value, variance, position4, normal4, out_value, fn);
  if (rc != RT_OK) return rc;
  c = lead_ctx(c);
  DeviceGuard guard;
  const size_t n = (size_t)p->base.width * p->base.height;
  // (the guides first: the kernels load them as float4, and the start of the staging buffer is aligned for that.  The device
  // copies of the outputs are planes of their own, so an in-place call needs no bounce there)
  IoSlot io[6] = {{(void*)position4, n * 16, true}, {(void*)normal4, n * 16, true}, {(void*)value, n * 4, true},
                  {(void*)variance, n * 4, true},   {out_value, n * 4, false},      {out_variance, n * 4, false}};
  return run_blocking(c, &c->filter, io, 6, [&] {
    return enqueue_filter_variance(c, *p, (const float*)io[2].dev, (const float*)io[3].dev, (const float4*)io[0].dev,
                                   (const float4*)io[1].dev, (float*)io[4].dev, (float*)io[5].dev, c->stream);
  });
}

int rt_trace_rays_device(rt_ctx* c, int32_t what, const void* d_rays6, const void* d_radius_sq, int64_t nray, void* d_out_tri,
                         void* d_out10, void* hip_stream) {
  const int rc = check_query_args(c, what, d_rays6, d_radius_sq, nray, d_out_tri, "rt_trace_rays_device");
  if (rc != RT_OK || nray == 0) return rc;
  DeviceGuard guard;
  return enqueue_query(lead_ctx(c), what, (const float*)d_rays6, (const float*)d_radius_sq, (long)nray, (int*)d_out_tri,
                       (float*)d_out10, (hipStream_t)hip_stream);
}

int rt_trace_rays(rt_ctx* c, int32_t what, const float* rays6, const float* radius_sq, int64_t nray, int32_t* out_tri, float* out10) {
  const int rc = check_query_args(c, what, rays6, radius_sq, nray, out_tri, "rt_trace_rays");
  if (rc != RT_OK || nray == 0) return rc;
  c = lead_ctx(c);
  DeviceGuard guard;
  const bool shadow = what == RT_TRACE_IN_SHADOW;
  const size_t n = (size_t)nray;
  IoSlot io[4] = {{(void*)rays6, n * 24, true}, {shadow ? (void*)radius_sq : nullptr, n * 4, true}, {out_tri, n * 4, false},
                  {shadow ? nullptr : out10, n * 40, false}};
  return run_blocking(c, &c->query, io, 4, [&] {
    return enqueue_query(c, what, (const float*)io[0].dev, (const float*)io[1].dev, (long)nray, (int*)io[2].dev, (float*)io[3].dev, c->stream);
  });
}

int rt_debug_trace_stats(rt_ctx* c, uint64_t out[8]) { return read_stats(c, &rt_ctx::query, 2, out); }

int rt_shade_points_device(rt_ctx* c, const void* d_points6, const void* d_seeds, int64_t npoints, const float light[3],
                           void* d_out_light, void* d_out_unshadowed, void* hip_stream) {
  const int rc = check_lit_args(c, d_points6, npoints, light, d_out_light, "rt_shade_points_device", "npoints");
  if (rc != RT_OK || npoints == 0) return rc;
  DeviceGuard guard;
  return enqueue_shade(lead_ctx(c), (const float*)d_points6, (const int*)d_seeds, (long)npoints, light, (float*)d_out_light,
                       (int*)d_out_unshadowed, (hipStream_t)hip_stream);
}

int rt_shade_points(rt_ctx* c, const float* points6, const int32_t* seeds, int64_t npoints, const float light[3], float* out_light,
                    int32_t* out_unshadowed) {
  int rc = check_lit_args(c, points6, npoints, light, out_light, "rt_shade_points", "npoints");
  if (rc == RT_OK) rc = check_seeds(seeds, npoints, "rt_shade_points");
  if (rc != RT_OK || npoints == 0) return rc;
  c = lead_ctx(c);
  DeviceGuard guard;
  const size_t n = (size_t)npoints;
  IoSlot io[4] = {{(void*)points6, n * 24, true}, {(void*)seeds, n * 4, true}, {out_light, n * 4, false}, {out_unshadowed, n * 4, false}};
  return run_blocking(c, &c->shade, io, 4, [&] {
    return enqueue_shade(c, (const float*)io[0].dev, (const int*)io[1].dev, (long)npoints, light, (float*)io[2].dev, (int*)io[3].dev, c->stream);
  });
}

int rt_debug_shade_stats(rt_ctx* c, uint64_t out[8]) { return read_stats(c, &rt_ctx::shade, 3, out); }

int rt_radiance_rays_device(rt_ctx* c, const void* d_rays6, const void* d_seeds, int64_t nray, const float light[3],
                            void* d_out_rgba4, void* d_out_prim, void* hip_stream) {
  const int rc = check_lit_args(c, d_rays6, nray, light, d_out_rgba4, "rt_radiance_rays_device", "nray");
  if (rc != RT_OK) return rc;
  if (((uintptr_t)d_out_rgba4 & 15) != 0) { set_error("rt_radiance_rays_device: d_out_rgba4 is not 16-byte aligned"); return RT_E_INVALID; }
  if (nray == 0) return rc;
  DeviceGuard guard;
  return enqueue_radiance(lead_ctx(c), (const float*)d_rays6, (const int*)d_seeds, (long)nray, light, (float*)d_out_rgba4,
                          (int*)d_out_prim, (hipStream_t)hip_stream);
}

int rt_radiance_rays(rt_ctx* c, const float* rays6, const int32_t* seeds, int64_t nray, const float light[3], float* out_rgba4,
                     int32_t* out_prim) {
  int rc = check_lit_args(c, rays6, nray, light, out_rgba4, "rt_radiance_rays", "nray");
  if (rc == RT_OK) rc = check_seeds(seeds, nray, "rt_radiance_rays");   // the domain of global_id, as for rt_shade_points
  if (rc != RT_OK || nray == 0) return rc;
  c = lead_ctx(c);
  DeviceGuard guard;
  const size_t n = (size_t)nray;
  // (the colours first: the kernels store them as float4, and the start of the staging buffer is aligned for that)
  IoSlot io[4] = {{out_rgba4, n * 16, false}, {(void*)rays6, n * 24, true}, {(void*)seeds, n * 4, true}, {out_prim, n * 4, false}};
  return run_blocking(c, &c->rad, io, 4, [&] {
    return enqueue_radiance(c, (const float*)io[1].dev, (const int*)io[2].dev, (long)nray, light, (float*)io[0].dev, (int*)io[3].dev, c->stream);
  });
}

int rt_debug_radiance_stats(rt_ctx* c, uint64_t out[8]) { return read_stats(c, &rt_ctx::rad, -1, out); }

int rt_render_aov_device(rt_ctx* c, const float rot[12], const float cam[3], float focal, int32_t sample,
                         const rt_aov_buffers* device_out, void* hip_stream) {
  const int rc = check_aov_args(c, rot, cam, device_out, "rt_render_aov_device");
  if (rc != RT_OK) return rc;
  const bool whole = !c->kids.empty();
  DeviceGuard guard;
  const AovPlanes A{device_out->prim, device_out->depth, (float4*)device_out->position4, (float4*)device_out->normal4,
                    (float4*)device_out->albedo4, (float4*)device_out->direction4};
  return enqueue_aov(lead_ctx(c), rot, cam, focal, sample, A, whole, (hipStream_t)hip_stream);
}

int rt_render_aov(rt_ctx* c, const float rot[12], const float cam[3], float focal, int32_t sample, const rt_aov_buffers* host_out) {
  const int rc = check_aov_args(c, rot, cam, host_out, "rt_render_aov");
  if (rc != RT_OK) return rc;
  const bool whole = !c->kids.empty();
  const int rows = c->owned_rows;
  c = lead_ctx(c);
  DeviceGuard guard;
  const int aa = c->cfg.aa_x * c->cfg.aa_y;
  const size_t count = (size_t)rows * c->cfg.width * (sample == RT_AOV_ALL_SAMPLES ? aa : 1);
  if (count == 0) return RT_OK;
  IoSlot io[6] = {{host_out->prim, count * 4, false},       {host_out->depth, count * 4, false},
                  {host_out->position4, count * 16, false}, {host_out->normal4, count * 16, false},
                  {host_out->albedo4, count * 16, false},   {host_out->direction4, count * 16, false}};
  return run_blocking(c, &c->aov, io, 6, [&] {
    const AovPlanes A{(int*)io[0].dev, (float*)io[1].dev, (float4*)io[2].dev, (float4*)io[3].dev, (float4*)io[4].dev, (float4*)io[5].dev};
    return enqueue_aov(c, rot, cam, focal, sample, A, whole, c->stream);
  });
}

int rt_debug_aov_stats(rt_ctx* c, uint64_t out[8]) {
  const int rc = read_stats(c, &rt_ctx::aov, 2, out);
  if (rc == RT_OK) out[6] = out[7] = 0;       // (the kernel's queue head lives behind the counters)
  return rc;
}

}  // extern "C"
