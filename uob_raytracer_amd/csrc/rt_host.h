// rt_host.h — what the host side of the library shares: the context, the error text, and the prototypes of the host
// functions that the kernel files define.  Included by the API files (rt_api.hip, rt_scene.hip, rt_calls.hip, rt_tile_sort.hip) AND by
// the kernel files that define launch_* and friends, so the compiler checks every prototype against its definition.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>
#include <utility>
#include <vector>

#include "rt_device.h"

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      uobrt::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return RT_E_DEVICE;                                                               \
    }                                                                                   \
  } while (0)

namespace uobrt {

void set_error(const char* fmt, ...);      // the text behind rt_last_error (rt_api.hip)

// Keeps the calling thread's error text across clean-up calls that may set their own: taken here, put back when the scope ends
struct KeepError {
  std::string text;
  KeepError();
  ~KeepError();
};

constexpr int kMaxTriangles = 4000000;     // the largest scene rt_init, an update or a replace accepts
constexpr int kWorldGrid = 32;             // world cells per axis of the mesh kernel's shadow-ray tile masks

// rt_kernel_generic.hip
void launch_generic(const FrameParams& P, bool count, hipStream_t stream);
bool generic_needs_records(int n);
void launch_stage_records(const FrameParams& P, hipStream_t stream);
void launch_trace_rays(const FrameParams& P, int what, const float* d_rays, const float* d_r2, long nray, int* d_tri,
                       float* d_out10, hipStream_t stream);
// rt_kernel_wave.hip
void launch_wave(const FrameParams& P, bool cull, bool count, bool prof, hipStream_t stream);
bool wave_kernel_supports(const FrameParams& P);
bool wave_takes_seed(const FrameParams& P, bool cull);
bool wave_can_count(const FrameParams& P, bool cull);
int wave_blocks_per_cu(bool leave_room);
// rt_kernel_mesh.hip
void launch_mesh(const FrameParams& P, bool count, bool prof, hipStream_t stream, hipStream_t aux, hipEvent_t ev_fork, hipEvent_t ev_join);
void launch_bin_primary(const FrameParams& P, hipStream_t stream);
bool mesh_kernel_supports(const FrameParams& P);
int mesh_tiles(int n);
int mesh_occ_words(int grid);
int mesh_screen_cells(int pixels);
int mesh_blocks_per_cu();
// rt_scene_update.hip
int launch_scene_check(const float4* v, const float4* col, int n, unsigned int* out, hipStream_t stream);
void launch_scene_refit(const float4* v, const float4* nrm, const float4* col, const int* orig, int n, float4* vm, float4* nm,
                        float4* cm, float4* tile_box, hipStream_t stream);
// rt_scene_pose.hip: the rest pose and one xform12 per object into a posed scene (vertices, normals)
constexpr unsigned int kPoseStatic = 0xffffu;   // object_of[i] of a triangle in no object (so at most 65535 objects)
void launch_pose(const float4* rest_v, const float4* rest_n, const unsigned short* object_of, const float* d_xforms12, int n,
                 float4* out_v, float4* out_n, hipStream_t stream);
// the rest pose and one xform12 per bone, blended by the influence table of the triangles [first, first + count)
void launch_skin(const float4* rest_v, const float4* rest_n, const ushort4* index, const float4* weights, const float* d_bones12,
                 int n, int first, int count, float4* out_v, float4* out_n, hipStream_t stream);
// rt_tile_build.hip: the tiled order of tiled_order(.., morton = true), on the device
size_t tile_build_scratch_bytes(int n);
int launch_tile_build(const float4* v, int n, const float lo[3], const float hi[3], int* orig, void* scratch, hipStream_t stream);
// rt_ray_query.hip
int query_stats_words();
void launch_query(const FrameParams& P, bool tiled, int what, const float* d_rays, const float* d_r2, long nray, int* d_tri,
                  float* d_out10, unsigned long long* stats, int cus, hipStream_t stream);
// rt_shade.hip
int shade_stats_words();
void launch_shade(const FrameParams& P, bool tiled, const float* d_points6, const int* d_seeds, long npoints, float* d_light,
                  int* d_cnt, unsigned long long* stats, int cus, hipStream_t stream);
// rt_radiance.hip
int radiance_stats_words();
size_t radiance_record_bytes(long nray);
void launch_radiance(const FrameParams& P, bool tiled, const float* d_rays6, const int* d_seeds, long nray, float4* d_rgba,
                     int* d_prim, float4* d_records, unsigned long long* stats, int cus, hipStream_t stream);
// rt_aov.hip
int aov_stats_words();
void launch_aov(const FrameParams& P, bool tiled, const AovPlanes& A, int sample, unsigned long long* stats, int cus, hipStream_t stream);
// rt_filter.hip: the a-trous filter of per-pixel planes (include/uob_rt.h rt_filter_plane).  A tile is kFilterTX
// contiguous pixels of kFilterTY rows; passes of spacing <= kFilterMaxTiledSpacing stage their taps in LDS (rows s apart), the
// others take them from the caches.  form: Tuning::filter_form
constexpr int kFilterTX = 64, kFilterTY = 4, kFilterMaxTiledSpacing = 32;
constexpr int kFilterFormBuiltIn = 0, kFilterFormDirect = 1;
int filter_stats_words();
void launch_filter_pack(const float4* d_pos, const float4* d_nrm, long count, int passes, float4* d_rec, unsigned long long* stats,
                        hipStream_t stream);
void launch_filter_pass(const rt_filter_params& p, int pass, int form, const float4* d_rec, const float* d_src, float* d_dst,
                        unsigned long long* stats, hipStream_t stream);
void launch_filter_counters(unsigned long long* stats, hipStream_t stream);
// filter_host.cpp: the ranges of rt_filter_params and the plane pointers, before anything else is looked at
int filter_check(const rt_filter_params* p, const void* value, const void* position4, const void* normal4, const void* out,
                 const char* fn);
// rt_filter_variance.hip: the variance-guided filter (include/uob_rt.h rt_filter_plane_variance, DESIGN.md 4.8a').  It shares
// the tile, the guide packing and the layout of the counters (filter_stats_words) with rt_filter.hip; its tiled form stages a
// third plane, so the largest spacing it serves is its own constant.  Per pass: the thresholds T from the variance, then the
// pass (d_src, d_vsrc) -> (d_dst, d_vdst)
constexpr int kFilterVarianceMaxTiledSpacing = 32;
void launch_filter_variance_threshold(const rt_filter_variance_params& vp, const float4* d_rec, const float* d_var, float* d_T,
                                      hipStream_t stream);
void launch_filter_variance_pass(const rt_filter_variance_params& vp, int pass, int form, const float4* d_rec, const float* d_T,
                                 const float* d_src, const float* d_vsrc, float* d_dst, float* d_vdst, unsigned long long* stats,
                                 hipStream_t stream);
void launch_filter_variance_counters(unsigned long long* stats, hipStream_t stream);
// filter_variance_host.cpp: the ranges of rt_filter_variance_params and the plane pointers, before anything else is looked at
int filter_variance_check(const rt_filter_variance_params* p, const void* value, const void* variance, const void* position4,
                          const void* normal4, const void* out_value, const char* fn);
// rt_accumulate.hip: the temporal reprojection of per-pixel planes (include/uob_rt.h rt_accumulate_plane): one
// launch over the plane in the filter's tiles (kFilterTX x kFilterTY adjacent pixels) and one that sums the counters
// d_rpos / d_rnrm: the reprojection planes of rt_accumulate_plane_moving, both or neither (then the launch is the plain entry's)
int accumulate_stats_words();
void launch_accumulate(const rt_accumulate_params& p, const float* d_value, const float4* d_pos, const float4* d_nrm, const int* d_prim,
                       const float4* d_rpos, const float4* d_rnrm, const float4* d_prev, float4* d_next, float* d_out_mean,
                       float* d_out_variance, unsigned long long* stats, hipStream_t stream);
// accumulate_host.cpp: the ranges of rt_accumulate_params and the plane pointers, before anything else is looked at
int accumulate_check(const rt_accumulate_params* p, const void* value, const void* position4, const void* normal4, const void* prev,
                     const void* next, const char* fn);
int accumulate_reproj_check(const void* reproj_position4, const void* reproj_normal4, const char* fn);
// rt_motion.hip: where each element's surface point was in the snapshot's scene (include/uob_rt.h rt_motion_planes, DESIGN.md
// 4.8c): one launch over the elements, kMotionBlocksX workgroups of 256 per grid.x (HIP keeps grid.x * block.x below 2^32;
// this is 2^30 elements) and the rest in grid.y, and one launch that sums the counters.  blocks_x: Tuning::motion_blocks_x
constexpr int kMotionBlocksX = 1 << 22;
int motion_stats_words();
void launch_motion(const float4* d_v_now, const float4* d_v_then, const float4* d_n_then, int n, const int* d_prim, const float4* d_pos,
                   const float4* d_nrm, long count, float4* d_out_pos, float4* d_out_nrm, int blocks_x, unsigned long long* stats,
                   hipStream_t stream);
// motion_host.cpp: the element planes and their count, before anything else is looked at
int motion_check(const void* prim, const void* position4, const void* normal4, int64_t count, const void* out_prev_position4,
                 const void* out_prev_normal4, const char* fn);
// rt_tile_sort.hip: the vertices' box, and the mesh kernel's tiled order and per-tile data (host arithmetic)
void vertex_box(const float* vertices4, int n, float lo[3], float hi[3]);
std::vector<int> tiled_order(const float* v4, int n, bool morton);
std::vector<float> tile_data_host(const float* v4, const int* orig, int n);

// ceil(2^32 / d): the magic number of rt_device.h div_magic (0 stands for d == 1)
inline uint32_t div_magic_for(int d) { return d > 1 ? (uint32_t)((0x100000000ull + (uint64_t)d - 1) / (uint64_t)d) : 0u; }

// Resident workgroups per CU of `kernel` launched with `threads` per workgroup and its static LDS (a persistent grid), asked
// of the current device at every launch: nothing is cached across contexts, devices or threads
inline int blocks_per_cu(const void* kernel, int threads) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess || per_cu < 1) per_cu = 2;
  return per_cu;
}
// The workgroups of a grid that has work for `want` and room for `cap`: never none
inline unsigned grid_blocks(long want, long cap) { return (unsigned)(want < cap ? (want > 0 ? want : 1) : cap); }

// Tuning knobs, read from the environment ONCE per context (rt_init); 0 / false = the built-in choice
struct Tuning {
  int job_tasks = 0;          // UOB_RT_JOB_TASKS: 64-ray tasks per job of the wave kernel
  int heavy_factor4 = 8;      // UOB_RT_HEAVY_FACTOR4: a job is expensive above this / 4 times the average cost
  bool plain_order = false;   // RT_FLAG_PLAIN_ORDER or UOB_RT_PLAIN_ORDER
  bool full_grid = false;     // UOB_RT_FULL_GRID: a rank of a multi-GPU job fills every wave slot too
  float l1_inflate = 3.5f;    // UOB_RT_L1_INFLATE: width of the point set level 1 bounds, in units of the task's own spread (1 .. 64)
  bool heavy_dilate = true;   // UOB_RT_HEAVY_DILATE=0: expensive jobs are listed without their row neighbours
  bool no_specialise = false; // UOB_RT_NO_SPECIALISE: the generic wave-kernel instantiation also where a specialised one exists
  int grid_per_cu = 0;        // UOB_RT_GRID_PER_CU: workgroups per CU of the wave kernel's persistent grid (experiments)
  bool phase_profile = false; // UOB_RT_PHASE_PROFILE: rt_count_executed returns s_memtime shares per phase
  bool timeline = false;      // UOB_RT_TIMELINE: the wave kernel records when its waves start and end (rt_debug_wave_timeline)
  int mask_debug = 0;         // UOB_RT_MASK_DEBUG: mesh kernel, switch single tile-mask stages off (fault isolation)
  bool tile_morton = false;   // UOB_RT_TILE_ORDER=morton: the mesh kernel's tiles in plain Morton order (tiled_order)
  int filter_form = 0;        // UOB_RT_FILTER_FORM=direct: every filter pass takes its taps from the caches (tools/filter_time.py)
  int motion_blocks_x = 0;    // UOB_RT_MOTION_BLOCKS_X: workgroups per grid.x of the motion kernel (1 .. 2^22; tests of its grid.y)
  bool no_seed = false;       // UOB_RT_NO_SEED=1: no tile-seed pre-pass, every job of the wave kernel starts unseeded
  int seed_rows = 16;         // UOB_RT_SEED_ROWS: rows of a seed tile (1 .. 64); the default is the default band height
  // what the pre-pass keeps (rt_device.h FrameParams seed_*_cap; the defaults by profiles/tile_seed_wide_ab.txt).  (1, 0, 0)
  // keeps what the strict rule kept, and a blocked level 1
  int seed_kp = 64;           // UOB_RT_SEED_KP: most triangles of a primary part (1 .. 64)
  int seed_casters = 32;      // UOB_RT_SEED_CASTERS: most casters off h's plane of a shadow part (0 .. 64)
  bool seed_sph = true;       // UOB_RT_SEED_SPH: keep shadow parts that name a sphere candidate
};

// ---- owners of device objects: move-only, and no device is stored — whoever frees on a given device sets
// it first, and a local owner is declared after the function's DeviceGuard.  g_live is what the owners of this process hold
// right now: allocations, their bytes, events, streams (rt_debug_live_device_objects)
inline std::atomic<int64_t> g_live[4];
inline void live_add(int slot, int64_t d) { g_live[slot].fetch_add(d, std::memory_order_relaxed); }

// A device array of T.  reset() is a plain hipFree: it waits for whatever still uses the memory.
template <class T>
struct DevMem {
  T* p = nullptr;
  size_t bytes = 0;
  DevMem() = default;
  DevMem(DevMem&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  DevMem& operator=(DevMem&& o) noexcept {     // frees what it held
    if (this != &o) { reset(); p = std::exchange(o.p, nullptr); bytes = std::exchange(o.bytes, 0); }
    return *this;
  }
  ~DevMem() { reset(); }
  hipError_t alloc(size_t count) {             // count elements; none: one byte, so that the pointer is never null
    reset();
    const size_t want = count ? count * sizeof(T) : 1;
    const hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) { p = nullptr; return e; }
    bytes = want; live_add(0, 1); live_add(1, (int64_t)want);
    return hipSuccess;
  }
  void reset() {
    if (p) { hipFree(p); live_add(0, -1); live_add(1, -(int64_t)bytes); }
    p = nullptr; bytes = 0;
  }
  operator T*() const { return p; }
};
// What every failed alloc answers
inline int alloc_failed() { set_error("hipMalloc failed: %s", hipGetErrorString(hipGetLastError())); return RT_E_NOMEM; }
// A byte buffer that only ever grows (ensure_bytes, rt_calls.hip)
using DevBuffer = DevMem<char>;
int ensure_bytes(DevBuffer* b, size_t bytes);

// An event or a stream, created with the flags of hipEventCreateWithFlags / hipStreamCreateWithFlags (none: hipEventCreate's)
template <class H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H), int Slot>
struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(Handle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept { if (this != &o) { reset(); h = std::exchange(o.h, nullptr); } return *this; }
  ~Handle() { reset(); }
  hipError_t create(unsigned flags = 0) {
    reset();
    const hipError_t e = Create(&h, flags);
    if (e != hipSuccess) h = nullptr; else live_add(Slot, 1);
    return e;
  }
  void reset() { if (h) { Destroy(h); live_add(Slot, -1); h = nullptr; } }
  operator H() const { return h; }
};
using Event = Handle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy, 2>;
using Stream = Handle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy, 3>;

// What a context owns of the buffers that depend on the scene's size or kernel family.  The context's working pointers
// (rt_ctx::d_verts_m, d_records, d_screen_masks, d_heavy, d_mesh_cost, ...) are these or nullptr: "is there a tiled copy",
// "are there tile masks" are asked of the working pointers everywhere, so a scene replaced by one of another family
// (rt_replace_scene) switches them and keeps the memory.  Everything sized by n holds rt_ctx::cap triangles.
struct SceneStore {
  DevMem<float4> verts_m, normals_m, colors_m, tile_box, records;
  DevMem<int> orig;
  DevMem<unsigned long long> screen_masks, world_masks;
  DevMem<unsigned int> world_occ;
  DevMem<unsigned int> heavy[2], heavy_flags, mesh_cost, mesh_order;
};

// One family of calls beside the frame (rt_calls.hip): ray queries, shade calls, radiance calls, AOV passes.
// Who waits for whose event is DESIGN.md 4.9; wait_scene_readers and wait_aov below are the only places that say it.
struct SideCall {
  Event ev;                                // recorded behind the latest call, created on first use
  bool pending = false;                    // a call has been enqueued: ev is worth waiting for
  DevMem<unsigned long long> d_stats;      // the latest call's work counters (+ its kernels' queue heads)
  int tiles = 0;                           // tiles of the latest call's scene (0: no tiled copy)
  DevBuffer io;                            // the blocking host entry: device copies of the caller's host arrays
};

}  // namespace uobrt

// What a context holds of the device is held by owners and goes with it; the raw device pointers are aliases of the store
struct rt_ctx {
  ~rt_ctx();                       // rt_api.hip: the children, the device, no work of the context still running
  rt_config cfg;
  uobrt::Tuning tune;
  int device = 0;
  int n = 0, n_shadow = 0;
  int cap = 0;                     // triangles the buffers sized by n hold: grows only (rt_replace_scene, rt_debug_scene_capacity)
  uobrt::SceneStore own;           // the owner of what a replaced scene may drop and regain
  uobrt::DevBuffer tile_scratch;   // rt_tile_build.hip: keys, indices and the digit table of the device tile build
  int owned_rows = 0;
  uobrt::DevMem<float4> d_verts, d_normals, d_colors;
  uobrt::DevMem<uint32_t> d_argb;  // internal framebuffer (stripe) for rt_render
  uobrt::DevMem<float4> d_rgb;     // lazily allocated float tap
  uobrt::DevMem<unsigned long long> d_counters;
  uobrt::DevMem<unsigned int> d_jobctr; // wave kernel's job queue heads
  // wave kernel: the tile seeds (rt_kernel_wave.hip rt_wave_seed), rewritten in front of every frame whose instantiation
  // takes them; sized by the frame's tiles on first use.  seed_* describe the table the last frame left (0 tiles: none)
  uobrt::DevMem<uobrt::SeedRec> d_seed;
  size_t seed_cap = 0;
  int seed_tile_rows = 0, seed_nseg = 0, seed_rows = 0;
  int cus = 256;                    // compute units of the device
  // wave kernel: last frame's expensive jobs go first (rt_device.h FrameParams::heavy_*); two lists, used in turn
  unsigned int *d_heavy[2] = {nullptr, nullptr}, *d_heavy_flags = nullptr;
  int heavy_cap = 0, heavy_phase = 0;
  size_t heavy_jobs_max = 0;       // entries of each of the two per-job flag arrays in d_heavy_flags
  // rt_register_output: a host range the device writes frames into directly
  char* reg_host = nullptr; char* reg_dev = nullptr; size_t reg_bytes = 0;
  bool reg_owner = false;        // this context called hipHostRegister (a child of a multi-device context only holds its device's alias)
  bool timeline_valid = false;   // the last frame left one (start, end, jobs) record per wave in d_timeline
  uobrt::DevMem<uint64_t> d_timeline;
  size_t timeline_waves = 0;
  uint32_t heavy_gen = 0;
  float4* d_records = nullptr;     // staged records in HBM for meshes beyond one LDS stage
  // mesh kernel (n > 64): the scene once more, reordered so that every 64-triangle tile is spatially compact (large
  // triangles first, then Morton order of the centroids), the original index of each triangle, and the tiles' boxes
  float4 *d_verts_m = nullptr, *d_normals_m = nullptr, *d_colors_m = nullptr, *d_tile_box = nullptr;
  int* d_orig = nullptr;
  uobrt::DevMem<uobrt::DevSphere> d_spheres;  // the sphere table in device memory (the wave-mapped kernels stage it into LDS)
  unsigned int *d_mesh_cost = nullptr, *d_mesh_order = nullptr;   // per 16x16-pixel block: last frame's cost, this frame's order
  bool mesh_order_valid = false;
  // mesh kernel: per-frame candidate-tile masks (rt_kernel_mesh.hip) and the scene's bounding box for its world grid
  unsigned long long *d_screen_masks = nullptr, *d_world_masks = nullptr;
  unsigned int* d_world_occ = nullptr;
  int nwords = 0, scx = 0, scy = 0;
  float box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0};
  float vbox_lo[3] = {0, 0, 0}, vbox_hi[3] = {0, 0, 0};   // the vertices' part of it (rt_update_spheres adds the new spheres)
  uobrt::Stream stream;
  uobrt::Stream aux_stream;                     // mesh kernel: the primary-ray masks are built beside the shadow-ray masks
  uobrt::Event ev_fork, ev_join;
  uobrt::Event ev0, ev1;
  bool timed = false;
  hipStream_t last_stream = nullptr;
  // several devices: one child context per entry of cfg.devices (then this context owns no device memory)
  std::vector<rt_ctx*> kids;
  uobrt::Event ev_go;               // parent: "the caller's stream has reached this frame"
  uobrt::Event ev_done;             // child: "this device's bands have been delivered"
  bool peer_ok = true;              // child: its device can copy 2-D into the destination device directly
  // rt_update_scene_device: the latest update, enqueued on the caller's stream; later frames (any stream) wait for it
  uobrt::Event ev_upd;
  bool upd_pending = false;
  uobrt::DevMem<unsigned int> d_check;  // rt_scene_check's result block (rt_scene_update.hip)
  // Rigid objects (rt_set_objects / rt_pose_objects*, rt_scene_pose.hip), on the context that poses (lead_ctx): the rest pose
  // and the per-triangle object table exist while nobj > 0; the staging scene (sized by cap) and the host entry's matrices
  // are kept once made
  int nobj = 0;
  uobrt::DevMem<float4> d_rest_verts, d_rest_normals;
  uobrt::DevMem<unsigned short> d_object_of;
  uobrt::DevBuffer pose_verts, pose_normals, pose_xforms;
  // A skin (rt_set_skin / rt_pose_skin*) shares the rest pose, the staging scene and the host entry's matrices with the
  // objects, so a context holds one or the other.  The influence table exists while skin_count > 0: per corner of the
  // triangles [skin_first, skin_first + skin_count) four bone indices (8 bytes) and four weights (16 bytes)
  int skin_first = 0, skin_count = 0, skin_nbones = 0;
  uobrt::DevMem<ushort4> d_skin_index;
  uobrt::DevMem<float4> d_skin_weights;
  // The scene's readers — ray queries (rt_ray_query.hip), shade calls (rt_shade.hip), radiance calls (rt_radiance.hip): they
  // read only the scene, so frames need not wait for them; later readers (they share the counters and staging of their
  // family) and scene updates do
  uobrt::SideCall query, shade, rad;
  uobrt::DevMem<float4> d_qrecords; // queries, no tiled copy, beyond one LDS stage: their own records (d_records is the frames')
  uobrt::DevBuffer rrec;                  // radiance calls: the records their first stage leaves for their second (both entries)
  // AOV passes (rt_aov.hip): frame-like — they use the frames' records and screen masks, so frames, updates and later
  // passes wait for the latest one; they touch none of the scheduling state above
  uobrt::SideCall aov;
  hipStream_t aov_stream = nullptr;   // (the caller's: not owned)
  // Filter calls (rt_filter.hip): they read no scene data and none of the buffers above, so they wait only for the filter
  // call before them (they share the scratch) and nothing but the next filter call and the destructor waits for them.
  // filter_guides: the packed guide records, 32 bytes per pixel; filter_planes: the two planes the passes alternate between
  // filter_variance: what a variance call (rt_filter_variance.hip) needs beyond that, 12 bytes per pixel: the two variance
  // planes and the thresholds; a context that only makes plain calls never allocates it
  uobrt::SideCall filter;
  uobrt::DevBuffer filter_guides, filter_planes, filter_variance;
  // Accumulate calls (rt_accumulate.hip): like the filter calls they read no scene data, wait only for the accumulate call
  // before them (they share the counters and the staging) and are waited for by the next one and the destructor.  They
  // need no scratch: the history buffers are the caller's
  uobrt::SideCall accum;
  // Motion calls (rt_motion.hip) and the snapshot they read (rt_motion_snapshot): the live scene in original order as the
  // previous view saw it, vertices [3 * motion_n] and normals [motion_n]; the buffers exist from the first snapshot to
  // rt_motion_release and only grow.  motion_taken: there is a snapshot, of motion_n triangles.  Snapshots and motion calls are one family of scene
  // readers (wait_scene_readers): they wait for a pending edit and for each other, and edits wait for them
  uobrt::SideCall motion;
  uobrt::DevMem<float4> motion_verts, motion_normals;
  int motion_n = 0;
  bool motion_taken = false;
};

namespace uobrt {

// Keeps the calling thread's current device unchanged across an API call (the caller may be a torch process)
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
  ~DeviceGuard() { if (prev >= 0) hipSetDevice(prev); }
};

// The single-device context that answers for a handle: devices[0] of a multi-device context, else the context itself
inline rt_ctx* lead_ctx(rt_ctx* c) { return c->kids.empty() ? c : c->kids[0]; }

// Frames and diagnostics read the scene that the context's latest rt_update_scene_device left, on whichever stream they run
inline hipError_t wait_scene(const rt_ctx* c, hipStream_t s) {
  return c->upd_pending ? hipStreamWaitEvent(s, c->ev_upd, 0) : hipSuccess;
}

// Whatever shares the frames' per-frame buffers (records, screen masks) or rewrites the scene waits for the latest AOV pass
inline hipError_t wait_aov(const rt_ctx* c, hipStream_t s) {
  return (c->aov.pending && s != c->aov_stream) ? hipStreamWaitEvent(s, c->aov.ev, 0) : hipSuccess;
}

// Whatever rewrites the scene, or shares a reader family's counters and staging, waits for the latest call of every
// reader family.  The ONE place that lists them: a new family of readers is added here and nowhere else.
inline int wait_scene_readers(const rt_ctx* c, hipStream_t s) {
  for (const SideCall* k : {&c->query, &c->shade, &c->rad, &c->motion})
    if (k->pending) HIP_TRY(hipStreamWaitEvent(s, k->ev, 0));
  return RT_OK;
}

// rt_api.hip: what a frame's kernels are given, and the same for what looks at the scene only
void fill_params(const rt_ctx* c, const float rot[12], const float cam[3], const float light[3], float focal, FrameParams* P);
void use_tiled_scene(const rt_ctx* c, FrameParams* P);
void scene_params(const rt_ctx* c, const float light[3], bool tiled, FrameParams* P);
// rt_scene.hip: what rt_init needs of the scene — the bounds of its arguments, the sphere table, the first scene
int validate_spheres(const rt_sphere* sph, int num);
int validate_vertices(const float* vertices4, int n);
int upload_spheres(rt_ctx* c);
int scene_first(rt_ctx* c, const float* v4, const float* n4, const float* c4, int n);

}  // namespace uobrt
