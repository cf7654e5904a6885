// rt_scene.hip — the scene of a context, first and later: rt_init's first scene (scene_first), same-count updates
// (rt_update_scene*), replacements of any count (rt_replace_scene*), rigid objects and skins posed from a rest pose
// (rt_set_objects, rt_pose_objects*, rt_set_skin, rt_pose_skin*) and the sphere table (rt_update_spheres).  Every triangle
// edit is one SceneEdit applied by scene_apply; a new kind of edit adds a source and an entry, not another copy of the flag
// logic.  No kernel lives here: the device work is rt_scene_update.hip (check, refit), rt_scene_pose.hip and
// rt_tile_build.hip; the host's tile sort is rt_tile_sort.hip.
#include <cmath>
#include <cstring>
#include <vector>

#include "rt_host.h"

using namespace uobrt;

// rt_init's and rt_update_spheres' bounds of a sphere table (the count is checked by the caller)
int uobrt::validate_spheres(const rt_sphere* sph, int num) {
  for (int i = 0; i < num; ++i) {
    const rt_sphere& s = sph[i];
    for (int k = 0; k < 3; ++k)
      if (!(fabsf(s.center[k]) <= kMaxCoordinate)) { set_error("sphere %d: |centre| must be finite and <= 2^16", i); return RT_E_INVALID; }
    if (!(fabsf(s.radius_sq) <= kMaxCoordinate * kMaxCoordinate)) { set_error("sphere %d: radius_sq must be finite and <= 2^32", i); return RT_E_INVALID; }
  }
  return RT_OK;
}

// Coordinate bound: the range over which the exact culls are verified and which keeps every
// determinant of the intersection tests below 2^126, where the v_rcp_f32 + Newton reciprocal equals IEEE
// division bit for bit (rt_math.h rcp_exact).
int uobrt::validate_vertices(const float* vertices4, int n) {
  for (size_t k = 0; k < (size_t)n * 12; ++k) {
    if ((k & 3) != 3 && !(fabsf(vertices4[k]) <= kMaxCoordinate)) {
      set_error("vertex %zu: coordinates must be finite and |x| <= 2^16", k / 4); return RT_E_INVALID;
    }
  }
  return RT_OK;
}

static int count_shadow_casters(const float* colors4, int n) {
  int cnt = 0;
  for (int i = 0; i < n; ++i) cnt += (colors4[4 * i + 3] != -1.0f);
  return cnt;
}

// The tiled copy into the context's buffers (scene_reserve has made them), on c->stream; blocking
static int upload_tiled(rt_ctx* c, const float* v4, const float* n4, const float* c4, const std::vector<int>& orig,
                        const std::vector<float>& box) {
  const int n = c->n, ntiles = mesh_tiles(n);
  std::vector<float> pv((size_t)n * 12), pn((size_t)n * 4), pc((size_t)n * 4);
  for (int j = 0; j < n; ++j) {
    const int i = orig[(size_t)j];
    memcpy(&pv[(size_t)12 * j], v4 + (size_t)12 * i, 48);
    memcpy(&pn[(size_t)4 * j], n4 + (size_t)4 * i, 16);
    memcpy(&pc[(size_t)4 * j], c4 + (size_t)4 * i, 16);
  }
  const size_t nb = (size_t)n * sizeof(float4);
  if (hipMemcpyAsync(c->d_verts_m, pv.data(), 3 * nb, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(c->d_normals_m, pn.data(), nb, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(c->d_colors_m, pc.data(), nb, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(c->d_orig, orig.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(c->d_tile_box, box.data(), (size_t)ntiles * 3 * sizeof(float4), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    set_error("scene upload failed: %s", hipGetErrorString(hipGetLastError())); return RT_E_DEVICE;
  }
  return RT_OK;
}

static int upload_tiled_scene(rt_ctx* c, const float* v4, const float* n4, const float* c4) {
  const std::vector<int> orig = tiled_order(v4, c->n, c->tune.tile_morton);
  return upload_tiled(c, v4, n4, c4, orig, tile_data_host(v4, orig.data(), c->n));
}

// The context's sphere table (cfg.spheres) into device memory; blocking
int uobrt::upload_spheres(rt_ctx* c) {
  const rt_config* cfg = &c->cfg;
  DevSphere tab[RT_MAX_SPHERES];
  memset(tab, 0, sizeof tab);
  for (int i = 0; i < cfg->num_spheres; ++i) {
    tab[i].cx = cfg->spheres[i].center[0]; tab[i].cy = cfg->spheres[i].center[1]; tab[i].cz = cfg->spheres[i].center[2];
    tab[i].r2 = cfg->spheres[i].radius_sq;
    memcpy(tab[i].col, cfg->spheres[i].color, 16);
  }
  if (hipMemcpy(c->d_spheres, tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess) {
    set_error("sphere table upload failed: %s", hipGetErrorString(hipGetLastError())); return RT_E_DEVICE;
  }
  return RT_OK;
}

// Every surface point lies on a triangle or a sphere: their bounding box, from the vertices' (the world grid of the
// mesh kernel's shadow-ray tile masks spans it: fill_params)
static void set_scene_box(rt_ctx* c, const float vlo[3], const float vhi[3]) {
  for (int k = 0; k < 3; ++k) { c->box_lo[k] = c->vbox_lo[k] = vlo[k]; c->box_hi[k] = c->vbox_hi[k] = vhi[k]; }
  const rt_config* cfg = &c->cfg;
  for (int i = 0; i < cfg->num_spheres; ++i) {
    const float r = sqrtf(fmaxf(cfg->spheres[i].radius_sq, 0.0f)) * 1.0001f + 1e-6f;
    for (int k = 0; k < 3; ++k) {
      c->box_lo[k] = fminf(c->box_lo[k], cfg->spheres[i].center[k] - r);
      c->box_hi[k] = fmaxf(c->box_hi[k], cfg->spheres[i].center[k] + r);
    }
  }
}

// An edit enqueued on `s` first waits for everything that may still read the buffers it overwrites: the context's
// previous frame (ev1, on whichever stream it ran), the calls that still read the scene, its latest AOV pass and its
// previous update
static int update_begin(rt_ctx* c, hipStream_t s) {
  HIP_TRY(hipSetDevice(c->device));
  if (c->timed) HIP_TRY(hipStreamWaitEvent(s, c->ev1, 0));
  if (wait_scene_readers(c, s) != RT_OK) return RT_E_DEVICE;
  HIP_TRY(wait_aov(c, s));
  HIP_TRY(wait_scene(c, s));
  return RT_OK;
}

// What the checks of a new scene derive from it, before any buffer is touched
struct SceneSummary {
  int n_shadow = 0;
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};   // the vertices' box
};

static void update_state(rt_ctx* c, const SceneSummary& sum) {
  c->n_shadow = sum.n_shadow;
  if (c->d_screen_masks) set_scene_box(c, sum.lo, sum.hi);
}

// ---- room for a scene: reserve on every device, then commit ------------------------------------------------------------
// Which buffers a scene of n triangles needs, by rt_init's rules
struct SceneNeeds {
  bool records, tiled, masks, heavy, mesh_sched;
};

static SceneNeeds scene_needs(const rt_ctx* c, int n) {
  const int f = c->cfg.flags;
  SceneNeeds q;
  q.records = n > 64;                                        // the staged records of the generic and mesh kernels
  q.tiled = n > 64 && !(f & RT_FLAG_GENERIC_KERNEL);         // the mesh kernel's tiled copy
  // candidate-tile masks: from 17 tiles on (with fewer, building and reading them costs more than the visits they save)
  q.masks = n > 16 * 64 && !(f & (RT_FLAG_NO_TILE_BINS | RT_FLAG_NO_CULL | RT_FLAG_GENERIC_KERNEL));
  q.heavy = n >= 1 && n <= 64 && !c->tune.plain_order;       // wave kernel: last frame's expensive jobs
  q.mesh_sched = q.tiled && !c->tune.plain_order;            // mesh kernel: last frame's block costs
  return q;
}

// New buffers of a scene that outgrows the context's capacity; they replace the old ones only in scene_commit, when every
// allocation of every device has succeeded
struct SceneGrowth {
  int cap = 0;                                               // 0: the scene fits, nothing to replace
  DevMem<float4> verts, normals, colors;
  SceneStore t;
};

// Everything a scene of n triangles needs that the context does not hold yet.  Nothing the context renders from is touched:
// what outgrows the capacity goes into *g; what the context meets for the first time (the buffers of a kernel family it has
// not run yet) goes into its store, which no frame reads before scene_select.  device_tiles: the device tile build will run
// (its scratch is made here and nowhere else).  For the count the context already holds, that scratch is all this allocates.
static int scene_reserve(rt_ctx* c, int n, bool device_tiles, SceneGrowth* g) {
  if (hipSetDevice(c->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", c->device); return RT_E_DEVICE; }
  const SceneNeeds q = scene_needs(c, n);
  const rt_config& cfg = c->cfg;
  SceneStore& o = c->own;
  SceneGrowth fresh;                           // reaches *g when everything has succeeded; a failure frees it on this device
  bool ok = true;
  auto get = [&](auto& m, size_t count) { if (ok && m.alloc(count) != hipSuccess) ok = false; };
  auto tiled_set = [&](SceneStore* t, size_t cap) {
    get(t->verts_m, 3 * cap); get(t->normals_m, cap); get(t->colors_m, cap); get(t->orig, cap);
    get(t->tile_box, (size_t)mesh_tiles((int)cap) * 3);
  };
  auto mask_set = [&](SceneStore* t, size_t cap) {
    const size_t nwords = (size_t)((mesh_tiles((int)cap) + 63) / 64), g3 = (size_t)kWorldGrid * kWorldGrid * kWorldGrid;
    get(t->screen_masks, (size_t)mesh_screen_cells(cfg.width) * mesh_screen_cells(cfg.height) * nwords);
    get(t->world_masks, g3 * nwords);
  };
  const bool grow = n > c->cap || !c->d_verts;
  const size_t cap = grow ? (n > 0 ? n : 1) : c->cap;
  if (grow) {    // (what the context already keeps for another family grows too: a later replace within capacity allocates nothing)
    fresh.cap = (int)cap;
    get(fresh.verts, 3 * cap); get(fresh.normals, cap); get(fresh.colors, cap);
    if (q.records || o.records) get(fresh.t.records, cap * kRecordsPerTriangle);
    if (q.tiled || o.verts_m) tiled_set(&fresh.t, cap);
    if (q.masks || o.screen_masks) mask_set(&fresh.t, cap);
  } else {
    if (q.records && !o.records) get(o.records, cap * kRecordsPerTriangle);
    if (q.tiled && !o.verts_m) tiled_set(&o, cap);
    if (q.masks && !o.screen_masks) mask_set(&o, cap);
  }
  if (q.masks && !o.world_occ) get(o.world_occ, (size_t)mesh_occ_words(kWorldGrid));
  if (q.heavy && !o.heavy_flags) {
    get(o.heavy[0], (size_t)c->heavy_cap); get(o.heavy[1], (size_t)c->heavy_cap); get(o.heavy_flags, 2 * c->heavy_jobs_max);
  }
  if (q.mesh_sched && !o.mesh_cost) {
    const size_t jobs = (size_t)((cfg.width + 15) / 16) * (size_t)((c->owned_rows + 15) / 16);
    // order list: up to four entries per block, + its length in the word behind it
    get(o.mesh_cost, jobs ? jobs : 1); get(o.mesh_order, 4 * (jobs ? jobs : 1) + 1);
  }
  if (!ok) return alloc_failed();
  if (device_tiles && q.tiled) {
    const int rc = ensure_bytes(&c->tile_scratch, tile_build_scratch_bytes((int)cap));
    if (rc != RT_OK) return rc;
  }
  if (q.masks && !c->aux_stream &&
      (c->aux_stream.create(hipStreamNonBlocking) != hipSuccess || c->ev_fork.create(hipEventDisableTiming) != hipSuccess ||
       c->ev_join.create(hipEventDisableTiming) != hipSuccess)) {
    set_error("stream/event creation failed"); return RT_E_DEVICE;
  }
  *g = std::move(fresh);
  return RT_OK;
}

// The grown buffers take the place of the old ones: every move assignment frees what the context held, and hipFree waits for
// whatever still uses what it frees.  From here to scene_select the context's working pointers are stale: the caller installs
// the new scene next, and nothing in between fails for a reason the caller could have (validation and allocation are behind it).
static void scene_commit(rt_ctx* c, SceneGrowth* g) {
  if (!g->cap) return;
  hipSetDevice(c->device);
  SceneStore &o = c->own, &t = g->t;
  c->d_verts = std::move(g->verts); c->d_normals = std::move(g->normals); c->d_colors = std::move(g->colors);
  o.records = std::move(t.records);
  o.verts_m = std::move(t.verts_m); o.normals_m = std::move(t.normals_m); o.colors_m = std::move(t.colors_m);
  o.orig = std::move(t.orig); o.tile_box = std::move(t.tile_box);
  o.screen_masks = std::move(t.screen_masks); o.world_masks = std::move(t.world_masks);
  c->d_qrecords.reset();                                     // (the queries make theirs on demand, for the capacity)
  c->cap = g->cap;
}

// The single-device contexts behind a handle
static std::vector<rt_ctx*> device_ctxs(rt_ctx* c) { return c->kids.empty() ? std::vector<rt_ctx*>(1, c) : c->kids; }

// Room for a scene of n triangles on every device of the handle, or no change at all
static int scene_reserve_all(rt_ctx* c, int n, bool device_tiles_wanted) {
  const std::vector<rt_ctx*> ks = device_ctxs(c);
  std::vector<SceneGrowth> grown(ks.size());
  for (size_t i = 0; i < ks.size(); ++i) {
    const int rc = scene_reserve(ks[i], n, device_tiles_wanted, &grown[i]);
    if (rc != RT_OK) {
      KeepError keep;
      for (size_t j = 0; j < i; ++j) { hipSetDevice(ks[j]->device); grown[j] = SceneGrowth(); }   // each freed on its device
      return rc;
    }
  }
  for (size_t i = 0; i < ks.size(); ++i) scene_commit(ks[i], &grown[i]);
  return RT_OK;
}

// ---- installing a scene on one device ----------------------------------------------------------------------------------
// The working pointers for a scene of n triangles: which kernel runs is decided from them, as rt_init decides it
static void scene_select(rt_ctx* c, int n) {
  const SceneNeeds q = scene_needs(c, n);
  const SceneStore& o = c->own;
  c->n = n;
  c->d_records = q.records ? o.records : nullptr;
  c->d_verts_m = q.tiled ? o.verts_m : nullptr; c->d_normals_m = q.tiled ? o.normals_m : nullptr;
  c->d_colors_m = q.tiled ? o.colors_m : nullptr; c->d_orig = q.tiled ? o.orig : nullptr; c->d_tile_box = q.tiled ? o.tile_box : nullptr;
  c->d_screen_masks = q.masks ? o.screen_masks : nullptr; c->d_world_masks = q.masks ? o.world_masks : nullptr;
  c->d_world_occ = q.masks ? o.world_occ : nullptr;
  c->nwords = q.masks ? (mesh_tiles(n) + 63) / 64 : 0;
  c->scx = q.masks ? mesh_screen_cells(c->cfg.width) : 0; c->scy = q.masks ? mesh_screen_cells(c->cfg.height) : 0;
  c->d_heavy[0] = q.heavy ? o.heavy[0] : nullptr; c->d_heavy[1] = q.heavy ? o.heavy[1] : nullptr;
  c->d_heavy_flags = q.heavy ? o.heavy_flags : nullptr;
  c->d_mesh_cost = q.mesh_sched ? o.mesh_cost : nullptr; c->d_mesh_order = q.mesh_sched ? o.mesh_order : nullptr;
}

// Switch the context to a scene of n triangles, on stream s behind update_begin.  The scheduling state is indexed by screen
// jobs and blocks, not by triangles: it is kept unless the scene crosses n = 64 (or is the first): then the next frame is a
// first frame, the state rt_init leaves.
static int scene_switch(rt_ctx* c, int n, bool first, hipStream_t s) {
  const bool restart = first || (c->n > 64) != (n > 64);
  scene_select(c, n);
  if (!restart) return RT_OK;
  c->mesh_order_valid = false;
  c->heavy_phase = 0; c->heavy_gen = 0;
  HIP_TRY(hipMemsetAsync(c->d_jobctr, 0, (2 * kJobHeads + 2) * kJobHeadStride * sizeof(unsigned int), s));
  if (c->d_heavy_flags) HIP_TRY(hipMemsetAsync(c->d_heavy_flags, 0, 2 * c->heavy_jobs_max * 4, s));
  return RT_OK;
}

// One edit of the triangles, whichever entry it came through
struct SceneEdit {
  const void *v, *nr, *col;   // float4 arrays [3n], [n], [n]; col == nullptr: the colours stay (a pose)
  bool on_device;             // device memory on the handle's device (enqueued on s), else host memory (blocking)
  int n;
  bool replace, first;        // replace: n may differ from the context's; first: rt_init's scene
  uint32_t flags;             // RT_UPDATE_*
  hipStream_t s;              // device source: the caller's stream
  SceneSummary sum;
};

// How an edit leaves the tiles of a context that keeps a tiled copy.  The tiling is a free choice (the closest hit resolves
// ties by the original index, d_orig), so the rt_init tiling can be kept and only the tiles' data recomputed:
//   source  replace  flags                    tiling
//   host    no       0                        refit only    (rt_scene_update.hip rt_scene_refit on the kept order)
//   host    no       RT_UPDATE_REORDER        host sort     (as rt_init: kd or Morton by the context's tuning)
//   host    no       RT_UPDATE_DEVICE_TILES   device build  (Morton order, rt_tile_build.hip; refit follows)
//   host    yes      0 or RT_UPDATE_REORDER   host sort     (there is no order to keep)
//   host    yes      RT_UPDATE_DEVICE_TILES   device build
//   device  no       0                        refit only
//   device  no       RT_UPDATE_DEVICE_TILES   device build
//   device  yes      0 or _DEVICE_TILES       device build
//   device  any      RT_UPDATE_REORDER        host sort: scene_apply stages the scene to host memory first
// (check_scene_flags has rejected both flags together)
enum class Tiling { HostSort, DeviceBuild, RefitOnly };

static Tiling choose_tiling(bool on_device, bool replace, uint32_t flags) {
  if (flags & RT_UPDATE_REORDER) return Tiling::HostSort;
  if (flags & RT_UPDATE_DEVICE_TILES) return Tiling::DeviceBuild;
  if (!replace) return Tiling::RefitOnly;
  return on_device ? Tiling::DeviceBuild : Tiling::HostSort;
}

// The edit (validated, room reserved) into one single-device context on stream s (of c->device); a device source lies on
// device src_dev.  A host source blocks; a device source leaves ev_upd for later frames to wait for.
static int scene_install_one(rt_ctx* c, const SceneEdit& e, Tiling tiling, int src_dev, hipStream_t s) {
  int rc = update_begin(c, s);
  if (rc != RT_OK) return rc;
  if (e.on_device && !c->ev_upd) HIP_TRY(c->ev_upd.create(hipEventDisableTiming));
  if (e.replace) { rc = scene_switch(c, e.n, e.first, s); if (rc != RT_OK) return rc; }
  auto copy = [&](float4* dst, const void* src, size_t bytes) {
    if (!src || !bytes) return hipSuccess;
    if (!e.on_device) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
    if (src_dev == c->device) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s);
    return hipMemcpyPeerAsync(dst, c->device, src, src_dev, bytes, s);   // the other devices of a handle: as the bands
  };
  const size_t nb = (size_t)e.n * sizeof(float4);
  HIP_TRY(copy(c->d_verts, e.v, 3 * nb));
  HIP_TRY(copy(c->d_normals, e.nr, nb));
  HIP_TRY(copy(c->d_colors, e.col, nb));
  if (c->d_verts_m && tiling == Tiling::HostSort) {          // (a host source: s is c->stream)
    rc = upload_tiled_scene(c, (const float*)e.v, (const float*)e.nr, (const float*)e.col);
    if (rc != RT_OK) return rc;
  } else if (c->d_verts_m) {
    if (tiling == Tiling::DeviceBuild &&     // Morton tiles on the device into d_orig
        launch_tile_build(c->d_verts, c->n, e.sum.lo, e.sum.hi, c->d_orig, c->tile_scratch.p, s) != 0) {
      set_error("tile build launch failed: %s", hipGetErrorString(hipGetLastError())); return RT_E_DEVICE;
    }
    launch_scene_refit(c->d_verts, c->d_normals, c->d_colors, c->d_orig, c->n, c->d_verts_m, c->d_normals_m, c->d_colors_m,
                       c->d_tile_box, s);
    HIP_TRY(hipGetLastError());
  }
  if (e.on_device) {
    HIP_TRY(hipEventRecord(c->ev_upd, s));
    c->upd_pending = true;
  } else {
    HIP_TRY(hipStreamSynchronize(s));
  }
  update_state(c, e.sum);
  return RT_OK;
}

// The edit into every device of the handle.  A host source: one device after the other, blocking.  A device source: a single
// device on the caller's stream; several devices each on its own stream after the caller's earlier work, copying from
// devices[0], and the caller's stream passes only when all have it.
static int scene_apply(rt_ctx* c, SceneEdit e) {
  const Tiling tiling = choose_tiling(e.on_device, e.replace, e.flags);
  std::vector<float> hv, hn, hc;
  if (e.on_device && tiling == Tiling::HostSort) {           // the tiles are sorted on the host: the scene goes through it
    hv.resize((size_t)e.n * 12); hn.resize((size_t)e.n * 4); hc.resize((size_t)e.n * 4);
    HIP_TRY(hipMemcpyAsync(hv.data(), e.v, hv.size() * 4, hipMemcpyDeviceToHost, e.s));
    HIP_TRY(hipMemcpyAsync(hn.data(), e.nr, hn.size() * 4, hipMemcpyDeviceToHost, e.s));
    HIP_TRY(hipMemcpyAsync(hc.data(), e.col ? e.col : lead_ctx(c)->d_colors, hc.size() * 4, hipMemcpyDeviceToHost, e.s));
    HIP_TRY(hipStreamSynchronize(e.s));
    e.v = hv.data(); e.nr = hn.data(); e.col = hc.data(); e.on_device = false;   // (e.sum stays: the device's)
  }
  int rc = scene_reserve_all(c, e.n, tiling == Tiling::DeviceBuild);
  if (rc != RT_OK) return rc;
  if (!e.on_device) {
    for (rt_ctx* k : device_ctxs(c)) { rc = scene_install_one(k, e, tiling, 0, k->stream); if (rc != RT_OK) break; }
  } else if (c->kids.empty()) {
    rc = scene_install_one(c, e, tiling, c->device, e.s);
  } else {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord(c->ev_go, e.s));
    for (rt_ctx* k : c->kids) {
      HIP_TRY(hipSetDevice(k->device));
      HIP_TRY(hipStreamWaitEvent(k->stream, c->ev_go, 0));
      rc = scene_install_one(k, e, tiling, c->device, k->stream);
      if (rc != RT_OK) break;
    }
    HIP_TRY(hipSetDevice(c->device));
    if (rc == RT_OK) for (rt_ctx* k : c->kids) HIP_TRY(hipStreamWaitEvent(e.s, k->ev_upd, 0));
  }
  // what a multi-device handle itself reports of the scene
  if (e.replace && !c->kids.empty()) { c->n = c->kids[0]->n; c->cap = c->kids[0]->cap; c->n_shadow = c->kids[0]->n_shadow; }
  return rc;
}

int uobrt::scene_first(rt_ctx* c, const float* v4, const float* n4, const float* c4, int n) {
  SceneEdit e = {v4, n4, c4, false, n, true, true, 0, nullptr, SceneSummary()};
  e.sum.n_shadow = count_shadow_casters(c4, n);
  if (scene_needs(c, n).masks) vertex_box(v4, n, e.sum.lo, e.sum.hi);
  return scene_apply(c, e);
}

// ---- the entries' checks -----------------------------------------------------------------------------------------------
static const uint32_t kUpdateFlags = RT_UPDATE_REORDER | RT_UPDATE_DEVICE_TILES;

static int check_scene_flags(uint32_t flags, const char* fn) {
  if (flags & ~kUpdateFlags) { set_error("%s: unknown flags 0x%x", fn, flags); return RT_E_INVALID; }
  if ((flags & kUpdateFlags) == kUpdateFlags) {
    set_error("%s: RT_UPDATE_REORDER (host tiles) and RT_UPDATE_DEVICE_TILES exclude each other", fn); return RT_E_INVALID;
  }
  return RT_OK;
}

// The arguments of rt_update_scene* (the count is the context's) and rt_replace_scene* (any count from 1 on)
static int check_scene_args(const rt_ctx* c, const void* v, const void* nr, const void* col, int32_t n, uint32_t flags,
                            const char* fn, bool replace) {
  const bool missing = !v || !nr || !col;
  if (replace) {
    if (!c) { set_error("%s: NULL context", fn); return RT_E_INVALID; }
    if (missing) { set_error("%s: scene arrays missing (NULL)", fn); return RT_E_INVALID; }
    if (n <= 0) { set_error("%s: n_new = %d, but a scene has at least one triangle", fn, n); return RT_E_INVALID; }
  } else {
    if (!c) { set_error("NULL context"); return RT_E_INVALID; }
    if (n != c->n) { set_error("%s: n = %d, but the context holds %d triangles", fn, n, c->n); return RT_E_INVALID; }
    if (n > 0 && missing) { set_error("scene arrays missing"); return RT_E_INVALID; }
  }
  const int rc = check_scene_flags(flags, fn);
  if (rc != RT_OK) return rc;
  if (n > kMaxTriangles) { set_error("triangle list of %d exceeds the supported maximum of %d", n, kMaxTriangles); return RT_E_UNSUPPORTED; }
  return RT_OK;
}

static float key_to_float(unsigned int k) {   // inverse of rt_scene_update.hip order_key
  const unsigned int u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// First pass of a device entry, on the caller's arrays: check the bound and reduce n_shadow and the box.  Returns once the
// result has been read back (this synchronises s); the context's buffers are untouched.
static int device_check(rt_ctx* c, const void* dv, const void* dc, int n, hipStream_t s, SceneSummary* sum) {
  HIP_TRY(hipSetDevice(c->device));
  if (!c->d_check) HIP_TRY(c->d_check.alloc(8));
  if (launch_scene_check((const float4*)dv, (const float4*)dc, n, c->d_check, s) != 0) {
    set_error("scene check launch failed: %s", hipGetErrorString(hipGetLastError())); return RT_E_DEVICE;
  }
  unsigned int res[8];
  HIP_TRY(hipMemcpyAsync(res, c->d_check, sizeof res, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (res[0] != 0u) { set_error("%u vertex coordinate(s) not finite or |x| > 2^16", res[0]); return RT_E_INVALID; }
  sum->n_shadow = (int)res[1];
  for (int k = 0; k < 3; ++k) { sum->lo[k] = key_to_float(res[2 + k]); sum->hi[k] = key_to_float(res[5 + k]); }
  return RT_OK;
}

// ---- rigid objects (rt_set_objects / rt_pose_objects*) and skins (rt_set_skin / rt_pose_skin*): DESIGN.md 4.2b, 4.2d --------
// The tables and the rest pose live on the context that poses (lead_ctx); a context holds an object table or a skin, which
// share the rest pose.  Nothing here runs for a context without either.
// (hipFree waits for a pose still reading what it frees)
static void drop_tables(rt_ctx* c, bool objects, bool skin) {
  rt_ctx* L = lead_ctx(c);
  if (objects) L->nobj = 0;
  if (skin) L->skin_first = L->skin_count = L->skin_nbones = 0;
  const bool rest = L->nobj == 0 && L->skin_count == 0;     // no table holds the rest pose any more
  if (!(objects && L->d_object_of) && !(skin && (L->d_skin_index || L->d_skin_weights)) &&
      !(rest && (L->d_rest_verts || L->d_rest_normals))) return;   // nothing to free: no HIP call
  DeviceGuard guard;
  hipSetDevice(L->device);
  if (objects) L->d_object_of.reset();
  if (skin) { L->d_skin_index.reset(); L->d_skin_weights.reset(); }
  if (rest) { L->d_rest_verts.reset(); L->d_rest_normals.reset(); }
}
static void drop_objects(rt_ctx* c) { drop_tables(c, true, false); }
static void drop_skin(rt_ctx* c) { drop_tables(c, false, true); }
// The scene behind the rest pose changes: whichever table the context holds goes
static void drop_poses(rt_ctx* c) { drop_tables(c, true, true); }

// The context's current scene becomes the rest pose (the buffers are made on first use and hold n triangles: whatever changes
// n drops both tables), on L's stream.  The snapshot waits for whatever still writes the scene, and for a pose still reading
// the old rest pose and the old table (an update's event): the caller's table upload follows on the same stream.
static int snapshot_rest(rt_ctx* L, const char* fn) {
  HIP_TRY(hipSetDevice(L->device));
  const size_t nb = (size_t)L->n * sizeof(float4);
  if ((!L->d_rest_verts && L->d_rest_verts.alloc(3 * (size_t)L->n) != hipSuccess) ||
      (!L->d_rest_normals && L->d_rest_normals.alloc((size_t)L->n) != hipSuccess))
    return alloc_failed();
  const int rc = update_begin(L, L->stream);
  if (rc != RT_OK) return rc;
  if (hipMemcpyAsync(L->d_rest_verts, L->d_verts, 3 * nb, hipMemcpyDeviceToDevice, L->stream) != hipSuccess ||
      hipMemcpyAsync(L->d_rest_normals, L->d_normals, nb, hipMemcpyDeviceToDevice, L->stream) != hipSuccess) {
    set_error("%s: snapshot failed: %s", fn, hipGetErrorString(hipGetLastError())); return RT_E_DEVICE;
  }
  return RT_OK;
}

static int check_pose_args(rt_ctx* c, const void* xforms, uint32_t flags, bool skin, const char* fn) {
  if (!c) { set_error("%s: NULL context", fn); return RT_E_INVALID; }
  if (!xforms) { set_error("%s: the matrices are missing (NULL)", fn); return RT_E_INVALID; }
  const int rc = check_scene_flags(flags, fn);
  if (rc != RT_OK) return rc;
  if (!skin && lead_ctx(c)->nobj == 0) {
    set_error("%s: the context has no object table (rt_set_objects first; a scene update or replace drops it)", fn);
    return RT_E_INVALID;
  }
  if (skin && lead_ctx(c)->skin_count == 0) {
    set_error("%s: the context has no skin (rt_set_skin first; a scene update or replace drops it)", fn);
    return RT_E_INVALID;
  }
  return RT_OK;
}

// The rest pose posed by the matrices at d_xforms12 (device memory of the lead device: one per object, or one per bone of the
// skin) into the staging scene, on s, and from there into the context as a device edit: the check runs on the staging scene,
// before anything live is written
static int pose_from_device(rt_ctx* c, const void* d_xforms12, uint32_t flags, bool skin, hipStream_t s) {
  rt_ctx* L = lead_ctx(c);
  HIP_TRY(hipSetDevice(L->device));
  const size_t nb = (size_t)L->cap * sizeof(float4);
  int rc = ensure_bytes(&L->pose_verts, 3 * nb);
  if (rc == RT_OK) rc = ensure_bytes(&L->pose_normals, nb);
  if (rc != RT_OK) return rc;
  // the staging scene may still be the source of the previous pose's copies, on whichever streams they run
  for (rt_ctx* k : device_ctxs(c)) HIP_TRY(wait_scene(k, s));
  if (skin)
    launch_skin(L->d_rest_verts, L->d_rest_normals, L->d_skin_index, L->d_skin_weights, (const float*)d_xforms12, L->n,
                L->skin_first, L->skin_count, (float4*)L->pose_verts.p, (float4*)L->pose_normals.p, s);
  else
    launch_pose(L->d_rest_verts, L->d_rest_normals, L->d_object_of, (const float*)d_xforms12, L->n, (float4*)L->pose_verts.p,
                (float4*)L->pose_normals.p, s);
  HIP_TRY(hipGetLastError());
  SceneEdit e = {L->pose_verts.p, L->pose_normals.p, nullptr, true, L->n, false, false, flags, s, SceneSummary()};
  rc = device_check(c, e.v, L->d_colors, e.n, s, &e.sum);
  if (rc != RT_OK) return rc;
  return scene_apply(c, e);
}

// rt_pose_objects and rt_pose_skin: the matrices (one per object / per bone) are uploaded, 48 bytes each; blocking
static int pose_from_host(rt_ctx* c, const float* xforms12, uint32_t flags, bool skin, const char* fn) {
  int rc = check_pose_args(c, xforms12, flags, skin, fn);
  if (rc != RT_OK) return rc;
  rt_ctx* L = lead_ctx(c);
  DeviceGuard guard;
  HIP_TRY(hipSetDevice(L->device));
  const size_t bytes = (size_t)(skin ? L->skin_nbones : L->nobj) * 12 * sizeof(float);
  rc = ensure_bytes(&L->pose_xforms, bytes);     // (only the blocking entries use the buffer: nothing can still be reading it)
  if (rc != RT_OK) return rc;
  HIP_TRY(hipMemcpyAsync(L->pose_xforms.p, xforms12, bytes, hipMemcpyHostToDevice, c->stream));
  rc = pose_from_device(c, L->pose_xforms.p, flags, skin, c->stream);
  if (rc != RT_OK) { KeepError keep; hipStreamSynchronize(c->stream); (void)hipGetLastError(); return rc; }
  HIP_TRY(hipStreamSynchronize(c->stream));      // (the stream of a multi-device handle has waited for every device)
  return RT_OK;
}

// rt_update_scene and rt_replace_scene: the arrays are checked once, before any device is touched
static int edit_from_host(rt_ctx* c, const float* v4, const float* n4, const float* c4, int32_t n, uint32_t flags, bool replace) {
  int rc = check_scene_args(c, v4, n4, c4, n, flags, replace ? "rt_replace_scene" : "rt_update_scene", replace);
  if (rc == RT_OK) rc = validate_vertices(v4, n);
  if (rc != RT_OK || n == 0) return rc;
  SceneEdit e = {v4, n4, c4, false, n, replace, false, flags, nullptr, SceneSummary()};
  e.sum.n_shadow = count_shadow_casters(c4, n);
  vertex_box(v4, n, e.sum.lo, e.sum.hi);
  DeviceGuard guard;
  drop_poses(c);                               // the scene behind the rest pose changes
  return scene_apply(c, e);
}

// rt_update_scene_device and rt_replace_scene_device: a first pass checks the bound and reduces n_shadow and the box; the
// live buffers, the object table and the skin stay untouched until it has passed
static int edit_from_device(rt_ctx* c, const void* dv, const void* dn, const void* dc, int32_t n, uint32_t flags, void* hip_stream,
                            bool replace) {
  int rc = check_scene_args(c, dv, dn, dc, n, flags, replace ? "rt_replace_scene" : "rt_update_scene", replace);
  if (rc != RT_OK || n == 0) return rc;
  DeviceGuard guard;
  SceneEdit e = {dv, dn, dc, true, n, replace, false, flags, (hipStream_t)hip_stream, SceneSummary()};
  rc = device_check(c, dv, dc, n, e.s, &e.sum);
  if (rc != RT_OK) return rc;
  drop_poses(c);
  return scene_apply(c, e);
}

extern "C" {

int rt_set_objects(rt_ctx* c, const int32_t* first, const int32_t* count, int32_t nobj) {
  if (!c) { set_error("rt_set_objects: NULL context"); return RT_E_INVALID; }
  if (nobj < 0 || nobj > (int32_t)kPoseStatic) { set_error("rt_set_objects: nobj = %d outside [0, 65535]", nobj); return RT_E_INVALID; }
  if (nobj > 0 && (!first || !count)) { set_error("rt_set_objects: first / count is NULL"); return RT_E_INVALID; }
  if (nobj == 0) { drop_objects(c); return RT_OK; }
  rt_ctx* L = lead_ctx(c);
  const int n = L->n;
  std::vector<unsigned short> object_of((size_t)n, (unsigned short)kPoseStatic);
  for (int k = 0; k < nobj; ++k) {
    const int f = first[k], cnt = count[k];
    if (cnt < 1 || f < 0 || f >= n || cnt > n - f) {
      set_error("rt_set_objects: object %d = [%d, %d + %d) is empty or not inside the context's %d triangles", k, f, f, cnt, n);
      return RT_E_INVALID;
    }
    for (int i = f; i < f + cnt; ++i) {
      if (object_of[(size_t)i] != kPoseStatic) {
        set_error("rt_set_objects: objects %d and %d overlap at triangle %d", (int)object_of[(size_t)i], k, i); return RT_E_INVALID;
      }
      object_of[(size_t)i] = (unsigned short)k;
    }
  }
  DeviceGuard guard;
  int rc = snapshot_rest(L, "rt_set_objects");
  if (rc == RT_OK && !L->d_object_of && L->d_object_of.alloc((size_t)n) != hipSuccess) rc = alloc_failed();
  if (rc == RT_OK &&
      (hipMemcpyAsync(L->d_object_of, object_of.data(), (size_t)n * sizeof(unsigned short), hipMemcpyHostToDevice, L->stream) != hipSuccess ||
       hipStreamSynchronize(L->stream) != hipSuccess)) {
    set_error("rt_set_objects: snapshot failed: %s", hipGetErrorString(hipGetLastError())); rc = RT_E_DEVICE;
  }
  if (rc != RT_OK) { KeepError keep; drop_poses(c); return rc; }
  L->nobj = nobj;
  drop_skin(c);                                  // (the rest pose stays: the objects hold it now)
  return RT_OK;
}

int rt_pose_objects(rt_ctx* c, const float* xforms12, uint32_t flags) {
  return pose_from_host(c, xforms12, flags, false, "rt_pose_objects");
}

int rt_pose_objects_device(rt_ctx* c, const void* d_xforms12, uint32_t flags, void* hip_stream) {
  const int rc = check_pose_args(c, d_xforms12, flags, false, "rt_pose_objects_device");
  if (rc != RT_OK) return rc;
  DeviceGuard guard;
  return pose_from_device(c, d_xforms12, flags, false, (hipStream_t)hip_stream);
}

int rt_set_skin(rt_ctx* c, int32_t first, int32_t count, const uint16_t* bone_index, const float* weights, int32_t nbones) {
  if (!c) { set_error("rt_set_skin: NULL context"); return RT_E_INVALID; }
  if (count == 0) { drop_skin(c); return RT_OK; }
  if (!bone_index || !weights) { set_error("rt_set_skin: bone_index / weights is NULL"); return RT_E_INVALID; }
  if (nbones < 1 || nbones > 65535) { set_error("rt_set_skin: nbones = %d outside [1, 65535]", nbones); return RT_E_INVALID; }
  rt_ctx* L = lead_ctx(c);
  const int n = L->n;
  // (the sign and the library's limit of the range first: they bound what the table checks read; then the table, then the
  // range against the context's scene)
  if (first < 0 || count < 0 || count > kMaxTriangles) {
    set_error("rt_set_skin: range [%d, %d + %d) is not a range of triangles (first >= 0, 0 <= count <= %d)", first, first, count,
              kMaxTriangles);
    return RT_E_INVALID;
  }
  const size_t corners = 3 * (size_t)count;
  for (size_t k = 0; k < corners; ++k)
    for (int j = 0; j < 4; ++j) {
      if ((int32_t)bone_index[4 * k + j] >= nbones) {
        set_error("rt_set_skin: corner %zu (triangle %zu): bone index %d is not below nbones = %d", k, (size_t)first + k / 3,
                  (int)bone_index[4 * k + j], nbones);
        return RT_E_INVALID;
      }
      if (!(weights[4 * k + j] >= 0.0f && weights[4 * k + j] <= 1.0f)) {
        set_error("rt_set_skin: corner %zu (triangle %zu): weight %g is not in [0, 1]", k, (size_t)first + k / 3,
                  (double)weights[4 * k + j]);
        return RT_E_INVALID;
      }
    }
  if (first >= n || count > n - first) {
    set_error("rt_set_skin: range [%d, %d + %d) is not inside the context's %d triangles", first, first, count, n);
    return RT_E_INVALID;
  }
  DeviceGuard guard;
  HIP_TRY(hipSetDevice(L->device));
  DevMem<ushort4> index;                         // the new table: the old one stays in force until everything has succeeded
  DevMem<float4> wts;
  if (index.alloc(corners) != hipSuccess || wts.alloc(corners) != hipSuccess)
    return alloc_failed();                       // (nothing of the context has been touched: its table and rest pose stay)
  int rc = snapshot_rest(L, "rt_set_skin");
  if (rc == RT_OK &&
      (hipMemcpyAsync(index, bone_index, corners * sizeof(ushort4), hipMemcpyHostToDevice, L->stream) != hipSuccess ||
       hipMemcpyAsync(wts, weights, corners * sizeof(float4), hipMemcpyHostToDevice, L->stream) != hipSuccess ||
       hipStreamSynchronize(L->stream) != hipSuccess)) {
    set_error("rt_set_skin: upload failed: %s", hipGetErrorString(hipGetLastError())); rc = RT_E_DEVICE;
  }
  if (rc != RT_OK) { KeepError keep; drop_poses(c); return rc; }   // (the snapshot has begun: the rest pose may be half written)
  L->d_skin_index = std::move(index); L->d_skin_weights = std::move(wts);   // (hipFree waits for a pose still reading the old table)
  L->skin_first = first; L->skin_count = count; L->skin_nbones = nbones;
  drop_objects(c);                               // (the rest pose stays: the skin holds it now)
  return RT_OK;
}

int rt_pose_skin(rt_ctx* c, const float* bones12, uint32_t flags) {
  return pose_from_host(c, bones12, flags, true, "rt_pose_skin");
}

int rt_pose_skin_device(rt_ctx* c, const void* d_bones12, uint32_t flags, void* hip_stream) {
  const int rc = check_pose_args(c, d_bones12, flags, true, "rt_pose_skin_device");
  if (rc != RT_OK) return rc;
  DeviceGuard guard;
  return pose_from_device(c, d_bones12, flags, true, (hipStream_t)hip_stream);
}

int rt_debug_skin_info(rt_ctx* c, int32_t* first, int32_t* count, int32_t* nbones) {
  if (!c || !first || !count || !nbones) { set_error("rt_debug_skin_info: NULL argument"); return RT_E_INVALID; }
  const rt_ctx* L = lead_ctx(c);
  *first = L->skin_first; *count = L->skin_count; *nbones = L->skin_nbones;
  return RT_OK;
}

int rt_debug_object_count(rt_ctx* c, int32_t* out) {
  if (!c || !out) { set_error("rt_debug_object_count: NULL argument"); return RT_E_INVALID; }
  *out = lead_ctx(c)->nobj;
  return RT_OK;
}

int rt_update_scene(rt_ctx* c, const float* vertices4, const float* normals4, const float* colors4, int32_t n, uint32_t flags) {
  return edit_from_host(c, vertices4, normals4, colors4, n, flags, false);
}

int rt_update_scene_device(rt_ctx* c, const void* d_vertices4, const void* d_normals4, const void* d_colors4, int32_t n,
                           uint32_t flags, void* hip_stream) {
  return edit_from_device(c, d_vertices4, d_normals4, d_colors4, n, flags, hip_stream, false);
}

int rt_replace_scene(rt_ctx* c, const float* vertices4, const float* normals4, const float* colors4, int32_t n_new, uint32_t flags) {
  return edit_from_host(c, vertices4, normals4, colors4, n_new, flags, true);
}

int rt_replace_scene_device(rt_ctx* c, const void* d_vertices4, const void* d_normals4, const void* d_colors4, int32_t n_new,
                            uint32_t flags, void* hip_stream) {
  return edit_from_device(c, d_vertices4, d_normals4, d_colors4, n_new, flags, hip_stream, true);
}

int rt_update_spheres(rt_ctx* c, const rt_sphere* spheres, int32_t num_spheres) {
  if (!c) { set_error("rt_update_spheres: NULL context"); return RT_E_INVALID; }
  if (num_spheres < 0 || num_spheres > RT_MAX_SPHERES) { set_error("rt_update_spheres: num_spheres must be in [0,%d]", RT_MAX_SPHERES); return RT_E_INVALID; }
  if (num_spheres > 0 && !spheres) { set_error("rt_update_spheres: spheres is NULL"); return RT_E_INVALID; }
  if (validate_spheres(spheres, num_spheres) != RT_OK) return RT_E_INVALID;
  DeviceGuard guard;
  auto set_cfg = [&](rt_ctx* k) {
    k->cfg.num_spheres = num_spheres;
    memset(k->cfg.spheres, 0, sizeof k->cfg.spheres);
    for (int i = 0; i < num_spheres; ++i) k->cfg.spheres[i] = spheres[i];
  };
  if (!c->kids.empty()) set_cfg(c);
  for (rt_ctx* k : device_ctxs(c)) {
    // the table is read by frames, readers and AOV passes: all of them first (a scene update), then a blocking copy
    const int rc = update_begin(k, k->stream);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipStreamSynchronize(k->stream));
    set_cfg(k);                                 // fill_params reads FrameParams::sph, nsph and the world grid's growth from it
    const int rc2 = upload_spheres(k);
    if (rc2 != RT_OK) return rc2;
    if (k->d_screen_masks) set_scene_box(k, k->vbox_lo, k->vbox_hi);   // the world grid spans the spheres too
  }
  return RT_OK;
}

int rt_debug_scene_capacity(rt_ctx* c, int64_t* out_triangles) {
  if (!c || !out_triangles) { set_error("rt_debug_scene_capacity: NULL argument"); return RT_E_INVALID; }
  *out_triangles = (int64_t)lead_ctx(c)->cap;
  return RT_OK;
}

int rt_debug_tile_data(rt_ctx* c, int32_t* orig, float* tiles, int32_t cap_tiles) {
  if (!c || cap_tiles < 0 || (cap_tiles > 0 && (!orig || !tiles))) { set_error("NULL argument"); return RT_E_INVALID; }
  c = lead_ctx(c);
  if (!c->d_tile_box) { set_error("rt_debug_tile_data: this context keeps no tiled copy of the scene"); return RT_E_UNSUPPORTED; }
  const int ntiles = mesh_tiles(c->n);
  if (cap_tiles == 0) return ntiles;
  if (cap_tiles < ntiles) { set_error("rt_debug_tile_data: room for %d tiles, %d needed", cap_tiles, ntiles); return RT_E_INVALID; }
  DeviceGuard guard;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(wait_scene(c, c->stream));
  HIP_TRY(hipMemcpyAsync(orig, c->d_orig, (size_t)c->n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(tiles, c->d_tile_box, (size_t)ntiles * 3 * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ntiles;
}

int rt_debug_scene_data(rt_ctx* c, float* vertices4, float* normals4, float* colors4, float* vertices4_m, float* normals4_m,
                        float* colors4_m, int32_t* n_shadow, float* vbox_lo, float* vbox_hi, int32_t cap_triangles) {
  if (cap_triangles < 0) { set_error("rt_debug_scene_data: capacity %d is negative", cap_triangles); return RT_E_INVALID; }
  if (!c) { set_error("rt_debug_scene_data: NULL context"); return RT_E_INVALID; }
  c = lead_ctx(c);
  const int n = c->n;
  if (cap_triangles == 0) return n;
  if (cap_triangles < n) { set_error("rt_debug_scene_data: room for %d triangles, %d needed", cap_triangles, n); return RT_E_INVALID; }
  if ((vertices4_m || normals4_m || colors4_m) && !c->d_verts_m) {
    set_error("rt_debug_scene_data: this context keeps no tiled copy of the scene"); return RT_E_UNSUPPORTED;
  }
  DeviceGuard guard;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(wait_scene(c, c->stream));
  const size_t nb = (size_t)n * sizeof(float4);
  auto fetch = [&](float* dst, const float4* src, size_t bytes) {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
  };
  HIP_TRY(fetch(vertices4, c->d_verts, 3 * nb));
  HIP_TRY(fetch(normals4, c->d_normals, nb));
  HIP_TRY(fetch(colors4, c->d_colors, nb));
  HIP_TRY(fetch(vertices4_m, c->d_verts_m, 3 * nb));
  HIP_TRY(fetch(normals4_m, c->d_normals_m, nb));
  HIP_TRY(fetch(colors4_m, c->d_colors_m, nb));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (n_shadow) *n_shadow = c->n_shadow;
  for (int k = 0; k < 3; ++k) {
    if (vbox_lo) vbox_lo[k] = c->vbox_lo[k];
    if (vbox_hi) vbox_hi[k] = c->vbox_hi[k];
  }
  return n;
}

}  // extern "C"
