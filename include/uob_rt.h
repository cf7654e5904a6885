/* uob_rt.h — C ABI of the MI355X-native Cornell-Box ray tracer (libuob_rt.so).
 *
 * This library replaces ONE path of harrywaugh/UOB_Raytracer: the OpenCL device boundary of
 * Source/skeleton.cpp — `opencl_initialise` (:366-497, build kernel + upload scene once) and
 * `offload_rendering` (:146-182, per-frame args + clEnqueueNDRangeKernel(draw) + blocking readback) —
 * and the kernel behind it, `draw` (Source/kernels.cl:368-428).  Plain pointers and sizes only; no C++
 * or torch types cross this boundary.  A maintainer's binding is shown in INTEGRATION.md.
 *
 * Conventions: every function returns RT_OK (0) or a negative RT_E_* code; the message for the last
 * failure on the calling thread is available from rt_last_error().  A context is not thread-safe
 * (the reference has one host thread and one in-order queue, skeleton.cpp:388), and its frames run one at a
 * time: a frame enqueued on another stream first waits for the context's previous frame.
 * State a context carries from frame to frame: the wave kernel hands out the row segments that were expensive
 * in the context's PREVIOUS frame first (scheduling only — no pixel depends on it; RT_FLAG_PLAIN_ORDER
 * switches it off).  Tuning knobs are read ONCE, in rt_init, from the environment (UOB_RT_JOB_TASKS,
 * UOB_RT_HEAVY_FACTOR4, UOB_RT_FULL_GRID, UOB_RT_TIMELINE, UOB_RT_TILE_ORDER: see DESIGN.md 4.1); nothing reads the
 * environment afterwards, rt_update_scene included.
 */
#ifndef UOB_RT_H
#define UOB_RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 2
#define RT_MAX_SPHERES 4
#define RT_MAX_DEVICES 8

enum {
  RT_OK = 0,
  RT_E_INVALID = -1,  /* bad argument / configuration                                            */
  RT_E_DEVICE = -2,   /* HIP runtime error (message carries hipGetErrorString)                   */
  RT_E_NOMEM = -3,
  RT_E_IO = -4,       /* file open/parse failure (OBJ loader, image writer)                      */
  RT_E_UNSUPPORTED = -5
};

/* One analytic sphere: kernels.cl:7-10 (sphere_centers / sphere_colors / sphere_radius_sqs).
 * color[3] is the material flag exactly like Triangle::color.w: >0 diffuse, 0 mirror, <0 glass.  */
typedef struct rt_sphere {
  float center[3];
  float radius_sq;
  float color[4];
} rt_sphere;

/* Every knob that the reference hard-codes as a #define/const (SURVEY.md §5 "Config / flags").
 * rt_config_default() fills in the reference's shipped values.                                   */
typedef struct rt_config {
  int32_t width, height;        /* SCREEN_WIDTH / SCREEN_HEIGHT, kernels.cl:16-17, skeleton.cpp:32-33 */
  int32_t aa_x, aa_y;           /* rays_x / rays_y, kernels.cl:12-13 (aa_rays = aa_x*aa_y); each 1..16        */
  int32_t shadow_samples;       /* light_sources, kernels.cl:316                                       */
  float   light_spread;         /* kernels.cl:317                                                      */
  int32_t max_bounces;          /* bounces, kernels.cl:343                                             */
  int32_t num_spheres;          /* SPHERES, kernels.cl:7 (0..RT_MAX_SPHERES)                           */
  rt_sphere spheres[RT_MAX_SPHERES];
  /* Row-band partition of the frame for multi-GPU rendering: this context owns the rows y with
   * (y / band_rows) % band_count == band_index, packed top to bottom in its output buffer.
   * band_count = 1 renders the whole frame.  Ray directions and the per-pixel RNG seed always use the
   * GLOBAL pixel coordinates (kernels.cl:378-380).                                                   */
  int32_t band_rows, band_index, band_count;
  int32_t device;               /* HIP device ordinal; -1 = current device                            */
  int32_t flags;                /* RT_FLAG_*                                                           */
  /* Several GPUs inside ONE context (one host thread, one stream per device — SURVEY.md 8(b) "Threading"):
   * with num_devices > 1 the rows this context owns are split into interleaved bands of device_band_rows
   * rows over devices[0..num_devices-1] (the same ordinal may be listed more than once), every device renders
   * its bands on its own stream, and rt_render / rt_render_device deliver the assembled frame exactly as a
   * single device would (bit-identical).  num_devices <= 1: `device` alone.  Needs band_count == 1.        */
  int32_t num_devices;
  int32_t devices[RT_MAX_DEVICES];
  int32_t device_band_rows;     /* 0 = 32                                                              */
} rt_config;

#define RT_FLAG_GENERIC_KERNEL 2u   /* always use the one-thread-per-pixel kernel (A/B and parity tests)  */
#define RT_FLAG_NO_CULL 4u          /* wave kernel: test every triangle for every surface point (no interval
                                       culling); output is bit-identical either way                        */
#define RT_FLAG_NO_TILE_BINS 8u     /* mesh kernel (n > 64): visit every 64-triangle tile instead of the per-frame
                                       candidate-tile masks; output is bit-identical either way                */
#define RT_FLAG_PLAIN_ORDER 16u     /* wave kernel: hand the jobs out in plain order every frame (no "last frame's
                                       expensive jobs first"): the context then carries no state from frame to frame */
#define RT_FLAG_STAGED_GATHER 32u   /* several devices: every device renders into its own stripe and the bands are
                                       copied to the destination, also for devices that could write it directly   */

typedef struct rt_ctx rt_ctx;

/* Per-frame work counters filled by rt_count_work (exact, reference early-exit semantics). */
typedef struct rt_work {
  uint64_t primary_rays, bounce_rays, shadow_rays;
  uint64_t closest_tri_tests, closest_sphere_tests;   /* batch_/single_ray_intersections loops    */
  uint64_t shadow_tri_tests, shadow_sphere_tests;     /* in_shadow loops incl. its early return   */
  uint64_t lit_hits;                                  /* direct_light invocations                 */
} rt_work;

/* ---- configuration -------------------------------------------------------------------------- */
/* Reference constants: 1024x1024, 2x2 AA, 10 shadow samples, spread 0.05, 10 bounces, the two live
 * spheres of kernels.cl:8-10, whole frame on the current device.                                     */
void rt_config_default(rt_config* cfg);
/* Number of rows / pixels of the frame owned by cfg's band selection.                                */
int32_t rt_config_owned_rows(const rt_config* cfg);

/* ---- the device boundary (replaces skeleton.cpp:366-497 and :146-182) ----------------------- */
/* Upload the scene once.  Arrays use the reference's packed layout (skeleton.cpp:474-484):
 * vertices4 = float4[3n] (w ignored), normals4 = float4[n] (w ignored), colors4 = float4[n] with
 * w = material flag.  The caller keeps ownership; data is copied before the call returns (as the
 * CL_TRUE writes at skeleton.cpp:486-496 do).                                                        */
int rt_init(const rt_config* cfg, const float* vertices4, const float* normals4, const float* colors4,
            int32_t n_triangles, rt_ctx** out_ctx);

/* Replace the context's triangles between frames (animated geometry).  Same packed layout and ownership as rt_init
 * (data copied before the call returns); n must equal the context's triangle count.  Later frames render the new scene
 * exactly as a context rt_init'ed with it would (bit-identical); the scheduling state ("last frame's expensive jobs
 * first") is kept.  Validation is rt_init's (finite, |x| <= 2^16); on any such error the context keeps its previous scene.
 * Meshes (n > 64): the tiles of rt_init are kept and their data recomputed on the device (refit), or, with
 * RT_UPDATE_REORDER, the triangles are sorted into tiles again on the host as rt_init does (DESIGN.md 4.2 "Scene updates").
 * The update waits for the context's previous frame, on whichever stream it runs; a multi-device context updates every
 * device.  Blocking.                                                                                               */
#define RT_UPDATE_REORDER 1u
int rt_update_scene(rt_ctx* ctx, const float* vertices4, const float* normals4, const float* colors4, int32_t n,
                    uint32_t flags);

/* Same, from device memory on the context's device (devices[0] of a multi-device context: the other devices receive the
 * scene by peer copy), enqueued on hip_stream (NULL = default stream) after the caller's earlier work on it.  A first pass
 * on the device checks the bound and reduces what the context keeps of the scene; the call returns once that has been
 * read back (this synchronises hip_stream up to that point) — the copies and the refit may still be running.  Later frames
 * of the context, on any stream, wait for them; the source buffers must not change until hip_stream has passed the
 * update.  RT_UPDATE_REORDER stages the scene through the host.                                                     */
int rt_update_scene_device(rt_ctx* ctx, const void* d_vertices4, const void* d_normals4, const void* d_colors4, int32_t n,
                           uint32_t flags, void* hip_stream);

/* RT_UPDATE_DEVICE_TILES (both entries above and both below; excludes RT_UPDATE_REORDER): the triangles are sorted into
 * tiles again ON THE DEVICE, large triangles first and the rest in Morton order of their centres — for a mesh that has
 * deformed far from its old tiles without leaving the GPU.  The order is the one rt_init makes under
 * UOB_RT_TILE_ORDER=morton, index for index; the kd split of rt_init's default order exists on the host only.      */
#define RT_UPDATE_DEVICE_TILES 2u

/* Replace the context's triangles by a scene of ANY count n_new >= 1 (rt_init's limits on n apply): objects appear and
 * disappear, a level of detail switches.  Same packed layout and ownership as rt_init.  After RT_OK every later operation
 * of the context — frames, AOV passes, ray queries, shade and radiance calls, the counting passes — gives exactly the bits
 * that a context rt_init'ed with the new scene, the context's current spheres and the same rt_config gives.  Which kernel
 * runs is decided as rt_init decides it, so a replace may cross n = 64 in either direction.  The registered output range,
 * the multi-device layout, the tuning read at rt_init and the staging of the calls beside the frame survive; so does the
 * scheduling state ("last frame's expensive jobs first") unless the scene crosses n = 64: then the next frame is a first
 * frame.  Validation is rt_init's (finite, |x| <= 2^16, count limits); on any validation or allocation error the context
 * keeps its previous scene, whole.  The buffers sized by n only grow: a replace that fits the capacity
 * (rt_debug_scene_capacity) allocates and frees none of them, and a smaller scene keeps the capacity.  The tiles of a mesh
 * are made on the host as rt_init makes them (RT_UPDATE_REORDER is accepted and changes nothing), or on the device with
 * RT_UPDATE_DEVICE_TILES.  Ordering as rt_update_scene: it waits for the context's previous frame and calls; a
 * multi-device context replaces the scene of every device.  Blocking.                                               */
int rt_replace_scene(rt_ctx* ctx, const float* vertices4, const float* normals4, const float* colors4, int32_t n_new,
                     uint32_t flags);

/* Same, from device memory on the context's device, enqueued on hip_stream exactly like rt_update_scene_device: the call
 * returns once the first pass (bound, n_shadow, box) has been read back; copies, the tile build and the refit may still be
 * running, nothing of the scene goes through host memory, and later operations of the context, on any stream, wait for
 * them on the device.  The tiles are made on the device (RT_UPDATE_DEVICE_TILES is implied); RT_UPDATE_REORDER asks for
 * the host's tiles instead and stages the scene through the host.  A scene beyond the capacity allocates new buffers and
 * frees the old ones, which synchronises the device.  If the check fails the context keeps its previous scene.        */
int rt_replace_scene_device(rt_ctx* ctx, const void* d_vertices4, const void* d_normals4, const void* d_colors4,
                            int32_t n_new, uint32_t flags, void* hip_stream);

/* Replace the sphere table (0..RT_MAX_SPHERES entries; centres, radii and materials may all change).  Validation is
 * rt_init's; on an error the context keeps its spheres.  Later operations see the new table exactly as a context
 * rt_init'ed with it in rt_config would.  Waits for the context's earlier work; blocking, tiny.                     */
int rt_update_spheres(rt_ctx* ctx, const rt_sphere* spheres, int32_t num_spheres);

/* Diagnostic: triangles the context's buffers can hold without allocating.                                          */
int rt_debug_scene_capacity(rt_ctx* ctx, int64_t* out_triangles);

/* ---- rigid objects: pose triangle ranges on the device from a rest pose (rt_scene_pose.hip) ----------
 * An OBJECT is a range [first, first + count) of the context's triangles, in the caller's original order.  A POSE is one
 * xform12 per object: 3 rows x (m_r0, m_r1, m_r2, t_r) — the layout of rot[12] with the translation in the pad column.
 * Posing the rest scene R with the poses X gives the scene P(R, X), rt_scene_transform's arithmetic (below):
 *   every vertex of an object's triangles becomes v'_r = ((v.x*m_r0 + v.y*m_r1) + v.z*m_r2) + t_r, FP32 without contraction;
 *   the normal of each such triangle is recomputed as rt_triangle_compute_normal does, always (also for an identity);
 *   triangles in no object, and all colours, are the rest scene's, bit for bit.
 * After RT_OK every later operation of the context — frames, AOV passes, ray queries, shade and radiance calls, the counting
 * passes — gives exactly the bits that rt_update_scene(ctx, pack(P(R, X)), flags) would have given.  A pose always starts
 * from R, never from the previous pose: nothing drifts.
 *
 * rt_set_objects snapshots the context's current scene (vertices, normals) as the rest pose R, in device memory, and records
 * the ranges: non-empty, inside [0, n), pairwise disjoint; nobj in 0 .. 65535.  nobj == 0 drops the table and frees the rest
 * pose.  Anything else is RT_E_INVALID, and the previous table survives.  Waits like rt_update_scene; blocking.  A context
 * that never calls it allocates nothing for it.  (A multi-device context keeps the rest pose on devices[0], which poses.)
 * rt_update_scene* and rt_replace_scene* change the scene behind the rest pose, so they drop the table; rt_update_spheres
 * does not touch it.  A pose call without a table is RT_E_INVALID.                                                          */
int rt_set_objects(rt_ctx* ctx, const int32_t* first, const int32_t* count, int32_t nobj);

/* Pose the objects: xforms12 = float32 [nobj][12] in host memory; nobj * 48 bytes are uploaded and nothing else.  The posed
 * scene is written on the device and goes through rt_update_scene_device's path: flags 0 refits into the existing tiles,
 * RT_UPDATE_DEVICE_TILES sorts the tiles again on the device, RT_UPDATE_REORDER makes host tiles and stages the posed scene
 * through the host.  Validation is rt_update_scene's, applied to the posed scene (finite, |x| <= 2^16): on any failure — a
 * NaN in a matrix, an object pushed out of range — the context keeps its previous scene, whole, and its rest pose.
 * Blocking.                                                                                                              */
int rt_pose_objects(rt_ctx* ctx, const float* xforms12, uint32_t flags);

/* Same, with the matrices in device memory on the context's device (devices[0]), e.g. the output of a simulation step;
 * stream-ordered exactly like rt_update_scene_device: the call returns once the first pass (bound, n_shadow, box) has been
 * read back, later operations of the context wait on the device, d_xforms12 may change once hip_stream has passed the call,
 * and nothing of the scene goes through host memory (unless RT_UPDATE_REORDER asks for it).  A multi-device context poses
 * on devices[0]; the other devices receive the posed scene by peer copy.                                                 */
int rt_pose_objects_device(rt_ctx* ctx, const void* d_xforms12, uint32_t flags, void* hip_stream);

/* Diagnostic: objects in the context's table (0: none).                                                              */
int rt_debug_object_count(rt_ctx* ctx, int32_t* out);

/* ---- skinned meshes: blend bone matrices per vertex on the device (rt_scene_pose.hip) ------------------
 * A SKIN is a range [first, first + count) of the context's triangles, in the caller's original order, with FOUR INFLUENCES
 * (bone j_k, weight w_k; k = 0..3) for each of its 3 * count corners: one row of bone_index [3*count][4] and of weights
 * [3*count][4] per corner, in the order corner 0, 1, 2 of triangle first, then of first + 1, and so on.  A POSE is one xform12
 * per bone (the layout of the rigid objects' xform12).  Skinning the rest scene R with the bones B gives the scene S(R, B),
 * rt_scene_skin's arithmetic (below): for every corner v of the range
 *   p_k   = the rigid pose of v by bone j_k, rt_scene_transform's expression: ((v.x*m_r0 + v.y*m_r1) + v.z*m_r2) + t_r per row r;
 *   v'_c  = ((w_0*p_0.c + w_1*p_1.c) + w_2*p_2.c) + w_3*p_3.c per component c;
 *   FP32 without contraction, in this operation order.  All four influences are always evaluated, also at weight 0: 0 * inf
 *   is a NaN, and the check of the posed scene rejects it.  Weights are not normalised: a sum below 1 pulls the vertex toward
 *   the origin.
 *   The normal of every triangle of the range is recomputed as rt_triangle_compute_normal does, always;
 *   triangles outside the range, and all colours, are the rest scene's, bit for bit.
 * After RT_OK every later operation of the context — frames, AOV passes, ray queries, shade and radiance calls, the counting
 * passes — gives exactly the bits that rt_update_scene(ctx, pack(S(R, B)), flags) would have given.  A pose always starts
 * from R, never from the previous pose: nothing drifts.
 *
 * rt_set_skin snapshots the context's current scene as the rest pose R exactly as rt_set_objects does (same buffers, same
 * waiting; blocking) and uploads the influence table, 24 bytes per corner.  Checked on the host before any device work: the
 * range is non-empty and inside [0, n); nbones in 1 .. 65535; every index < nbones; every weight finite and in [0, 1].
 * Anything else is RT_E_INVALID with a message that names the corner or the argument, and the previous table (skin or
 * objects) survives.  count == 0 drops the skin and frees its memory.  A context holds EITHER an object table OR a skin (they
 * share the rest pose): a successful rt_set_skin drops the objects, a successful rt_set_objects with nobj > 0 drops the skin.
 * rt_update_scene* and rt_replace_scene* drop the skin as they drop the objects; rt_update_spheres does not touch it.  A
 * context that never calls rt_set_skin allocates nothing for it.  rt_pose_skin* without a skin is RT_E_INVALID ("no skin"),
 * as rt_pose_objects* with only a skin is ("no object table").                                                             */
int rt_set_skin(rt_ctx* ctx, int32_t first, int32_t count, const uint16_t* bone_index, const float* weights, int32_t nbones);

/* Pose the skin: bones12 = float32 [nbones][12] in host memory; nbones * 48 bytes are uploaded and nothing else.  In every
 * other respect rt_pose_objects: the posed scene is written on the device and goes through rt_update_scene_device's path
 * (flags 0, RT_UPDATE_DEVICE_TILES or RT_UPDATE_REORDER, with the same meaning and the same exclusion); validation is that of
 * the posed scene (finite, |x| <= 2^16), and on any failure the context keeps its previous scene, whole, and its rest pose.
 * Blocking.                                                                                                              */
int rt_pose_skin(rt_ctx* ctx, const float* bones12, uint32_t flags);

/* Same, with the bones in device memory on the context's device (devices[0]), stream-ordered exactly like
 * rt_pose_objects_device / rt_update_scene_device: d_bones12 may change once hip_stream has passed the call.  A multi-device
 * context poses on devices[0]; the other devices receive the posed scene by peer copy.                                  */
int rt_pose_skin_device(rt_ctx* ctx, const void* d_bones12, uint32_t flags, void* hip_stream);

/* Diagnostic: the skinned range and the bone count of the context's skin (zeros: none).                              */
int rt_debug_skin_info(rt_ctx* ctx, int32_t* first, int32_t* count, int32_t* nbones);

/* Render one frame and read it back: rot = 3 rows x (x,y,z,pad) exactly as rot_matrix[12] at
 * skeleton.cpp:149-151; cam/light = first 12 bytes of camera_position / light_position (:162,:164);
 * focal = focal_length (:166), in units of AA sub-pixels along x.  out_argb receives
 * owned_rows*width ARGB8888 words (A=255, kernels.cl:39); out_rgb_f32 (nullable) receives the
 * pre-quantisation colour final/aa_rays as float4 (w=1) per pixel — the parity tap.  Synchronous,
 * like the CL_TRUE read at skeleton.cpp:179.                                                         */
int rt_render(rt_ctx* ctx, const float rot[12], const float cam[3], const float light[3], float focal,
              uint32_t* out_argb, float* out_rgb_f32);

/* Same frame, but the ARGB (and optional float4) output stays in device memory the caller owns
 * (e.g. a torch tensor handed to an RCCL gather).  Enqueued on `hip_stream` (a hipStream_t, may be
 * NULL for the default stream); returns without synchronising.  With several devices in the context
 * (rt_config.devices) the buffers must live on devices[0] and hip_stream must be a stream of that device: the other
 * devices' bands arrive by peer copy, ordered after the caller's earlier work on the stream and before its later work. */
int rt_render_device(rt_ctx* ctx, const float rot[12], const float cam[3], const float light[3],
                     float focal, void* d_out_argb, void* d_out_rgb_f32, void* hip_stream);

/* Exact work counters of the frame (un-timed instrumented pass; reference semantics).               */
int rt_count_work(rt_ctx* ctx, const float rot[12], const float cam[3], const float light[3],
                  float focal, rt_work* out);

/* Work the wave kernel actually EXECUTES for the frame (un-timed instrumented pass).  Fails with
 * RT_E_UNSUPPORTED for every frame the thread-per-pixel kernel renders — RT_FLAG_GENERIC_KERNEL; an empty scene
 * or one whose triangles are all glass; a mesh (n > 64) with RT_FLAG_NO_CULL or with more than 64 AA samples per
 * pixel; up to 64 triangles with more than 64 AA samples per pixel and either RT_FLAG_NO_CULL or more than 64
 * shadow samples — and for the wave-kernel frames that have no counting build: more than 64 shadow samples, or
 * more than 64 AA samples per pixel (the table at its head).  out[0] = surface points whose
 * samples were tested (level 3), out[1] = first-stage (t) sample-test passes = 64 sample tests each,
 * out[2] = second-stage (u,v) passes, out[3] = wave-wide sphere evaluations, out[4] = lit surface points
 * decided fully lit by the interval bounds, out[5] = 64-ray tasks that needed no sampling at all,
 * out[6..7] = 0.
 * Meshes (n > 64, tiled kernel): out[0] = (wave, tile) visits of the primary pass, out[1] = triangles left by
 * the primary bound over those visits, out[2] = (wave, tile) visits of the shadow pass, out[3] = triangles
 * left by level 1, out[4] = level-3 point-pair calls, out[5] = their first-stage passes, out[6] = the longest
 * 16x16-pixel block in s_memtime ticks (shader cycles), out[7] = task rounds per wave summed over waves.                                                                       */
int rt_count_executed(rt_ctx* ctx, const float rot[12], const float cam[3], const float light[3],
                      float focal, uint64_t out[8]);

/* Device time of the most recent rt_render / rt_render_device kernel(s) on this context in ms,
 * measured with hipEvents on the launch stream (synchronises that stream).                          */
int rt_last_kernel_ms(rt_ctx* ctx, float* out_ms);

/* Diagnostic: run the device functions of the path on caller-supplied rays (host arrays), one lane per ray,
 * against the context's scene and sphere table — the function-level golden vectors of the reference are checked
 * through this entry (tests/test_gpu_functions.py).  rays6 = nray x (start.xyz, direction.xyz).
 *   RT_TRACE_IN_SHADOW   : in_shadow (kernels.cl:243-311) with radius_sq[nray]  -> out_tri[k] = 0 / 1
 *   RT_TRACE_CLOSEST_HIT : single_ray_intersections (kernels.cl:168-241) -> out_tri[k] = -1 / -2 / triangle,
 *                          out10[10k..] = intersect.xyz, normal.xyz, colour.xyzw (zero on a miss)          */
enum { RT_TRACE_IN_SHADOW = 0, RT_TRACE_CLOSEST_HIT = 1 };
int rt_debug_trace_rays(rt_ctx* ctx, int32_t what, const float* rays6, const float* radius_sq, int64_t nray,
                        int32_t* out_tri, float* out10);

/* Ray queries (picking, line of sight, probes) on the context's scene as its latest update left it: the same `what` modes,
 * arrays and results as rt_debug_trace_rays (bit-identical), on a tile-culled kernel (rt_ray_query.hip).
 * rays6 = float32 [nray][6] (start, direction), 4-byte aligned; out10 is nullable for RT_TRACE_CLOSEST_HIT (written with
 * zeros on a miss) and not written for RT_TRACE_IN_SHADOW.  A NULL ctx / rays6 / out_tri, an unknown mode, nray < 0 and a
 * missing radius_sq in RT_TRACE_IN_SHADOW are RT_E_INVALID; nray == 0 is a no-op.  Queries write nothing a frame reads:
 * frames do not wait for them, and they do not wait for frames; the context's next query and scene update (and rt_destroy)
 * wait for them.  A multi-device context runs its queries on devices[0].
 * Host arrays, blocking.                                                                                                 */
int rt_trace_rays(rt_ctx* ctx, int32_t what, const float* rays6, const float* radius_sq, int64_t nray,
                  int32_t* out_tri, float* out10);
/* Device memory on the context's device (devices[0] of a multi-device context), enqueued on hip_stream (NULL = default
 * stream) after the caller's earlier work; returns without synchronising.                                                */
int rt_trace_rays_device(rt_ctx* ctx, int32_t what, const void* d_rays6, const void* d_radius_sq, int64_t nray,
                         void* d_out_tri, void* d_out10, void* hip_stream);
/* Diagnostic: work counters of the context's most recent rt_trace_rays / rt_trace_rays_device (synchronises it; zeros
 * before the first).  out[0] rays, out[1] 64-ray waves, out[2] tiles of the scene (0 without a tiled copy), out[3] (wave,
 * tile) pairs left by the bundle test, out[4] (wave, tile) pairs whose triangles were tested, out[5] lane-level triangle
 * tests, out[6] rays traced without culling (outside the certificates' domain; every ray without a tiled copy), out[7] 0. */
int rt_debug_trace_stats(rt_ctx* ctx, uint64_t out[8]);

/* ---- direct light at caller points (rt_shade.hip) -----------------------------------------------------
 * How much light arrives at a surface point: one channel of the reference's direct_light (kernels.cl:313-340; its three
 * channels are equal), the jittered area-light sum of the context's shadow_samples shadow rays with its light_spread, on the
 * context's scene as its latest update left it.  With rt_trace_rays and RT_TRACE_IN_SHADOW this completes the queries: what
 * does a ray hit, is a point shadowed, how much light arrives.
 *   points6 = float32 [npoints][6]: position.xyz, normal.xyz (ray.intersect and intersect_normal, e.g. the position4 /
 *             normal4 planes of rt_render_aov).
 *   seeds   = nullable int32 [npoints]: the global_id that seeds the point's jitter stream, 0 .. 2^24 (the frame uses the
 *             pixel id y * width + x); NULL = k & 0xFFFFFF.  rt_shade_points rejects a seed outside the domain with
 *             RT_E_INVALID before any device work; in rt_shade_points_device such a seed yields an unspecified light value
 *             (it only feeds the generator).
 *   out_light[k] = exactly the reference's bits: seeds (id, (uint)(id * 91.0f), (uint)(id * 19.0f)), one generator step, then
 *             per sample one step and the ray (start, dir + crush(r, light_spread)) with dir = light - P,
 *             start = P + 0.0001f * dir, radius_sq = (dx*dx + dy*dy) + dz*dz, tested by in_shadow;
 *             term = (16 * max(dot(dir, N), 0)) / (4 * pi_f * radius_sq) is added once per unblocked sample and 0.0f * term
 *             for a blocked one, in FP32 without contraction, then / shadow_samples — the frame's own summation, so that
 *             albedo.xyz * (0.5f + out_light) is the frame's colour of a diffuse primary hit.  Non-finite and degenerate
 *             inputs (P at the light) give what that arithmetic gives; points whose rays leave the domain of the exact culls
 *             (|coordinate| <= 2^16) are traced without culling.
 *   out_unshadowed[k] = nullable: the number of unblocked samples, 0 .. shadow_samples (a shadow matte's numerator).  When
 *             it is NULL a point whose term is 0 (facing away from the light) is not traced.
 * A NULL ctx / points6 / light / out_light and npoints < 0 or > 2^31 are RT_E_INVALID; npoints == 0 is a no-op.  Ordering is
 * rt_trace_rays': frames and shade calls do not wait for each other; the context's next query, shade call and scene update
 * (and rt_destroy) wait for a shade call, and it waits for the query and the update before it.  A multi-device context runs
 * it on devices[0].
 * rt_shade_points: host arrays, blocking (staged through device memory the context keeps and grows on demand).
 * rt_shade_points_device: device memory on the context's device, enqueued on hip_stream (NULL = default stream) after the
 * caller's earlier work; returns without synchronising.                                                                   */
int rt_shade_points(rt_ctx* ctx, const float* points6, const int32_t* seeds, int64_t npoints, const float light[3],
                    float* out_light, int32_t* out_unshadowed);
int rt_shade_points_device(rt_ctx* ctx, const void* d_points6, const void* d_seeds, int64_t npoints, const float light[3],
                           void* d_out_light, void* d_out_unshadowed, void* hip_stream);
/* Diagnostic: work counters of the context's most recent shade call (synchronises it; zeros before the first).  out[0] points,
 * out[1] sample rays traced, out[2] 64-lane waves of rays, out[3] tiles of the scene (0 without a tiled copy), out[4] (wave,
 * tile) pairs left by the bundle test (without a tiled copy: every run of 64 triangles), out[5] pairs whose triangles were
 * tested, out[6] lane-level triangle tests, out[7] points not traced because their term is 0.                             */
int rt_debug_shade_stats(rt_ctx* ctx, uint64_t out[8]);

/* ---- the frame's full colour for caller rays (rt_radiance.hip) ----------------------------------------
 * What rt_render computes for one AA sample of a pixel — closest hit, the reflect / refract bounce loop, soft-shadowed
 * direct light, the colour rule — for rays the caller supplies, on the context's scene as its latest update left it: any
 * camera the pinhole cannot express (panoramas, cube-map probes, fisheye and stereo rigs, lens samples for depth of field),
 * or the colour along a picking ray.  With the `direction` plane of rt_render_aov as the rays and the pixel ids as the seeds,
 * the per-pixel sum in sample order / aa is rt_render's out_rgb_f32, bit for bit, on every pixel.
 *   rays6   = float32 [nray][6]: start.xyz, direction.xyz (rt_trace_rays' layout).  The direction is used as given, not
 *             normalised.  A ray starts in air: medium AIR, colour w = 1, intersect_triangle = -1 (kernels.cl:400-405).
 *   seeds   = nullable int32 [nray]: the global_id of the ray's jitter stream, 0 .. 2^24 (the frame uses the pixel id
 *             y * width + x); NULL = k & 0xFFFFFF.  rt_radiance_rays rejects a seed outside the domain with RT_E_INVALID
 *             before any device work; in rt_radiance_rays_device such a seed yields an unspecified colour.
 *   out_rgba4 = float32 [nray][4], 16-byte aligned.  xyz is the colour:
 *             the first hit is single_ray_intersections (kernels.cl:168-241), the bits of rt_trace_rays(RT_TRACE_CLOSEST_HIT);
 *             miss: (0, 0, 0);
 *             diffuse hit (albedo w > 0; exactly: not w <= 0): albedo.xyz * (0.5f + L);
 *             mirror or glass hit (w <= 0): secondary_light (kernels.cl:342-365) with the context's max_bounces — while
 *             b < max_bounces and the hit's w <= 0: reflect_ray (w == 0) or refract_ray (w < 0; n = n1 / n2 in FP32, the
 *             medium carried from bounce to bounce), start = P + 0.0001f * dir with the UNnormalised new direction, then the
 *             direction normalised, closest hit again; at the first hit with w > 0 the colour is
 *             (0.9f * (0.5f + L)) * albedo.xyz, and (0, 0, 0) if the loop ends on a miss or runs out;
 *             L is exactly rt_shade_points' out_light for (that hit's position, its normal, the ray's seed, light), with the
 *             context's shadow_samples and light_spread.  FP32 without contraction, operation order of the reference.
 *             w is 1.0f when the first hit exists and 0.0f on a miss: coverage, for compositing over a background.
 *   out_prim  = nullable int32 [nray]: the first hit, -1 / -2 / the ORIGINAL triangle index (as rt_trace_rays' out_tri).
 * NaN and non-finite rays give what the arithmetic gives: they hit nothing, so the result is zero.  Rays outside the domain
 * of the exact culls (finite, |start| <= 2^16, 2^-20 <= max |direction component| <= 2^16) are traced without culling; that
 * holds for the bounce rays and the sample rays of a call as well.
 * A NULL ctx / rays6 / light / out_rgba4 and nray < 0 or > 2^31 are RT_E_INVALID, before any device work; nray == 0 is a
 * no-op.  Ordering is rt_shade_points': a radiance call touches none of the per-frame buffers, frames do not wait for it and
 * it does not wait for frames; it waits for the scene update, query, shade call and radiance call before it, and the
 * context's next query, shade call, radiance call and scene update (and rt_destroy) wait for it.  A multi-device context
 * runs it on devices[0].
 * rt_radiance_rays: host arrays, blocking (staged through device memory the context keeps and grows on demand).
 * rt_radiance_rays_device: device memory on the context's device, enqueued on hip_stream (NULL = default stream) after the
 * caller's earlier work; returns without synchronising, and no stage of it waits for the host: how many rays reach a diffuse
 * surface stays on the device.  The scratch between its stages (48 bytes per ray) belongs to the context and grows on
 * demand; only a call with more rays than any before it allocates.                                                       */
int rt_radiance_rays(rt_ctx* ctx, const float* rays6, const int32_t* seeds, int64_t nray, const float light[3],
                     float* out_rgba4, int32_t* out_prim);
int rt_radiance_rays_device(rt_ctx* ctx, const void* d_rays6, const void* d_seeds, int64_t nray, const float light[3],
                            void* d_out_rgba4, void* d_out_prim, void* hip_stream);
/* Diagnostic: work counters of the context's most recent radiance call (synchronises it; zeros before the first).  out[0]
 * rays, out[1] bounce rays traced, out[2] rays that reached a diffuse surface (shaded points), out[3] shadow sample rays
 * traced, out[4] (wave, tile) pairs whose triangles were tested by closest-hit walks, out[5] lane-level triangle tests of
 * closest-hit walks, out[6] lane-level triangle tests of shadow walks, out[7] rays of any kind traced without culling
 * (outside the certificates' domain).                                                                                     */
int rt_debug_radiance_stats(rt_ctx* ctx, uint64_t out[8]);

/* ---- AOV pass: what every pixel of a view sees (rt_aov.hip) ------------------------------------------
 * The planes describe the PRIMARY HIT of the frame that rt_render would render with the same rot, cam and focal on the
 * context's current scene (after rt_update_scene).  No light is involved.
 * Every pointer is nullable: a NULL plane is not computed / not written.  At least one must be set.                      */
typedef struct rt_aov_buffers {
  int32_t* prim;        /* -1 miss, -2 sphere, >= 0 ORIGINAL triangle index (as rt_trace_rays' out_tri)      */
  float*   depth;       /* 1 float: |P - cam| (definition below); +INFINITY on a miss                        */
  float*   position4;   /* float4: intersect.xyz, w = 1 on a hit; all zero on a miss                          */
  float*   normal4;     /* float4: intersect_normal.xyz, w = 0; all zero on a miss                            */
  float*   albedo4;     /* float4: intersect_color.xyzw (w = material flag: >0 diffuse, 0 mirror, <0 glass);
                           all zero on a miss                                                                 */
  float*   direction4;  /* float4: the primary ray's normalised direction, w = 0 (written hit or miss)        */
} rt_aov_buffers;

/* sample in 0 .. aa_x*aa_y-1 selects one AA sample per pixel, index dy*aa_x+dx exactly as the frame numbers them: every
 * plane then holds owned_rows * width elements in the frame's own pixel order (bands: the owned rows packed top to bottom;
 * ray directions use the global pixel coordinates).  sample == RT_AOV_ALL_SAMPLES: every plane holds
 * owned_rows * width * aa elements, the samples of a pixel adjacent, in sample order (an antialiased matte, a per-sample
 * denoiser).
 * prim, position4, normal4, albedo4 carry exactly the bits that rt_trace_rays(RT_TRACE_CLOSEST_HIT) returns for the ray
 * (cam, direction), i.e. the reference's single_ray_intersections (kernels.cl:168-241).  depth is derived from the
 * position: with d = P - cam component-wise in FP32, depth = sqrtf((d.x*d.x + d.y*d.y) + d.z*d.z), no contraction,
 * correctly rounded square root.
 * Ordering: a pass is a frame-like operation.  It runs one at a time with the context's frames and other passes (it shares
 * their per-frame buffers), waits for the scene update before it, and scene updates wait for it.  It leaves the scheduling
 * state ("last frame's expensive jobs first", block costs) and rt_last_kernel_ms untouched: a frame after a pass is
 * scheduled as if the pass had not happened.  A multi-device context runs the pass on devices[0] over all rows it owns.
 * Errors: a NULL ctx / rot / cam / buffers struct, all planes NULL and a sample out of range are RT_E_INVALID.
 * rt_render_aov: host planes, blocking; staged through device memory the context keeps and grows on demand.
 * rt_render_aov_device: planes in device memory on the context's device (devices[0]), enqueued on hip_stream (NULL =
 * default stream) after the caller's earlier work; returns without synchronising, like rt_render_device.                 */
#define RT_AOV_ALL_SAMPLES (-1)
int rt_render_aov(rt_ctx* ctx, const float rot[12], const float cam[3], float focal, int32_t sample,
                  const rt_aov_buffers* host_out);
int rt_render_aov_device(rt_ctx* ctx, const float rot[12], const float cam[3], float focal, int32_t sample,
                         const rt_aov_buffers* device_out, void* hip_stream);
/* Diagnostic: work counters of the context's most recent AOV pass (synchronises it; zeros before the first).  out[0] samples,
 * out[1] 64-lane waves, out[2] tiles of the scene (0 without a tiled copy), out[3] (wave, tile) pairs left by the screen
 * masks (every tile without masks), out[4] (wave, tile) pairs whose triangles were tested, out[5] lane-level triangle tests,
 * out[6..7] 0.                                                                                                          */
int rt_debug_aov_stats(rt_ctx* ctx, uint64_t out[8]);

/* ---- edge-stopping a-trous filter of per-pixel planes (rt_filter.hip) ----------------------------------
 * A geometry-guided reconstruction filter for a noisy per-pixel estimate (e.g. the visibility of a few shadow samples), run
 * over planes the library already produces.  It reads no scene data.  With binary edge stops, dyadic tap weights and a fixed
 * summation order it is a pure FP32 function of its inputs; every implementation (the device kernels, rt_filter_plane_host)
 * gives the same bits.
 * Planes of `height` rows x `width` pixels, row-major:
 *   value      float32 [h][w]      the plane to filter;
 *   position4  float32 [h][w][4]   the guides, in the layouts of rt_render_aov's position4 / normal4 planes.  A pixel is
 *   normal4    float32 [h][w][4]   VALID iff position4.w > 0 (a miss of the AOV pass has w = 0; a NaN is invalid).
 * V_0 = value.  For pass i = 0 .. passes-1 the tap spacing is s = 2^i, and for every pixel p = (x, y):
 *   - p not valid: V_{i+1}[p] = V_i[p] (its bits).
 *   - otherwise the 25 taps (dx, dy) in {-2..2}^2 are visited with dy outer and dx inner, both ascending; the tap pixel is
 *     q = (x + dx*s, y + dy*s) and the tap weight w = h[|dx|] * h[|dy|] with h = (3/8, 1/4, 1/16) (every product exact).
 *     The centre tap is always accepted.  Any other tap is accepted iff all of these hold, with P / N the xyz of position4 /
 *     normal4:
 *       1. q lies inside the plane and is valid;
 *       2. (Np.x*Nq.x + Np.y*Nq.y) + Np.z*Nq.z >= normal_min_dot;
 *       3. with d = Pq - Pp component-wise, fabsf((Np.x*d.x + Np.y*d.y) + Np.z*d.z) <= plane_eps;
 *       4. fabsf(V_i[q] - V_i[p]) <= value_max_diff * 2^-i (one product by the exact power of two; +INFINITY stays).
 *     All arithmetic is FP32 without contraction.  A comparison with a NaN operand is false, so a NaN tap is always rejected,
 *     also at value_max_diff = +INFINITY.
 *     Over the accepted taps in visiting order: num = num + w * V_i[q] (one multiply, one add) and den = den + w, both from
 *     +0 (den is exact in any order: every partial sum is a multiple of 1/256 not above 1).
 *     V_{i+1}[p] = V_i[p] (its bits) if only the centre was accepted (den == 9/64); otherwise num / den, correctly rounded,
 *     and when that quotient is a NaN (infinities of both signs among the accepted taps) the quiet NaN 0x7FC00000.
 * The output is V_passes.  The guides are those of the centre pixel and do not change between passes.
 * What follows exactly: a region of valid pixels whose values are all 1.0f (or all 0.0f) keeps them, since num == den
 * (num == 0); normal_min_dot = 2 with unit normals rejects every tap and returns the input bit for bit.  Equal values other
 * than those two need not survive bit for bit.                                                                            */
typedef struct rt_filter_params {
  int32_t width, height;     /* >= 1; width * height <= 2^31                          */
  int32_t passes;            /* 1 .. 8                                               */
  float   normal_min_dot;    /* not NaN                                              */
  float   plane_eps;         /* >= 0, not NaN                                        */
  float   value_max_diff;    /* >= 0 or +INFINITY, not NaN                           */
} rt_filter_params;
/* 5 passes, normal_min_dot 0.9, plane_eps 0.01, value_max_diff +INFINITY: defaults for a scene of the Cornell box's size
 * (about 2 units across).  They are stated, not tuned on images.                                                          */
void rt_filter_params_default(rt_filter_params* params, int32_t width, int32_t height);
/* out may be the same pointer as value (in place); any other overlap of the planes is the caller's error.  A NULL ctx, params
 * or plane, and any parameter outside the ranges above, are RT_E_INVALID with a message that names the field, before the
 * context is looked at and before any device work.  Ordering: a filter call is no reader of the scene — it does not wait
 * for updates, frames or the calls beside them, and they do not wait for it; it waits only for the context's previous
 * filter call (they share the scratch), and rt_destroy waits for it.  Ordering with whatever produces its input planes is
 * the caller's stream.  A multi-device context runs it on devices[0].
 * rt_filter_plane: host arrays, blocking (staged through device memory the context keeps and grows on demand).
 * rt_filter_plane_device: planes in device memory on the context's device, the guides 16-byte aligned, enqueued on hip_stream
 * (NULL = default stream) after the caller's earlier work; returns without synchronising, and no stage waits for the host.
 * The scratch (40 bytes per pixel: the packed guides and two planes the passes alternate between) belongs to the context and
 * only grows; only a call larger than any before it allocates, and a context that never filters allocates nothing for it.
 * Such a growing call (the first one included) is the exception to "does not wait": it frees the smaller scratch and
 * allocates the larger one before it enqueues anything, and freeing device memory synchronises the whole device, not only
 * the previous filter call.  A caller that must not stall filters its largest plane once at start-up.
 * UOB_RT_FILTER_FORM=direct in the environment of rt_init makes every pass take its taps from the caches (measurements).   */
int rt_filter_plane(rt_ctx* ctx, const rt_filter_params* params, const float* value, const float* position4,
                    const float* normal4, float* out);
int rt_filter_plane_device(rt_ctx* ctx, const rt_filter_params* params, const void* d_value, const void* d_position4,
                           const void* d_normal4, void* d_out, void* hip_stream);
/* Diagnostic: work counters of the context's most recent filter call (synchronises it; zeros before the first).  out[0] pixels,
 * out[1] passes, out[2] accepted taps summed over valid centres and passes (the centre included), out[3] valid pixels, out[4]
 * (valid pixel, pass) pairs that kept their value because only the centre was accepted, out[5] 0 (a count only after rt_filter_plane_variance,
 * below), out[6..7] 0.                                                                                                    */
int rt_debug_filter_stats(rt_ctx* ctx, uint64_t out[8]);
/* The same filter on the host (CPU only, no context): the statement the device kernels are pinned against.  Same checks. */
int rt_filter_plane_host(const rt_filter_params* params, const float* value, const float* position4, const float* normal4,
                         float* out);

/* ---- variance-guided a-trous filter (rt_filter_variance.hip, DESIGN.md 4.8a') -------------------------------------------
 * rt_filter_plane with the value stop of SVGF: besides the value it carries the value's variance (rt_accumulate_plane's
 * out_variance), and a tap is also rejected when its value differs from the centre's by more than sigma_value standard
 * deviations of the centre.  So a noisy pixel averages with its neighbours and a clean step keeps its edge, which one global
 * value_max_diff cannot tell apart.  A pure FP32 function of its inputs like rt_filter_plane; every implementation (the
 * device kernels, rt_filter_plane_variance_host) gives the same bits.
 * Planes as rt_filter_plane's, and variance float32 [h][w].  The definition is exactly rt_filter_plane's, carrying a second
 * plane Var_i with Var_0 = variance, with four differences.  All arithmetic is FP32 without contraction.
 *   1. Threshold.  For every pass i and valid pixel p: g starts at +0; the 3 x 3 taps (dx, dy) in {-1, 0, 1}^2 at spacing 1
 *      (not dilated by the pass) are visited with dy outer and dx inner, both ascending; k = 1/4 (centre), 1/8
 *      (|dx| + |dy| = 1), 1/16 (corners); c = Var_i[q] if q = (x + dx, y + dy) lies inside the plane and is valid, else
 *      Var_i[p]; g = g + k * c (one multiply, one add).  T = sigma_value * sqrtf(g) + value_eps: the correctly rounded square
 *      root, one multiply, one add.  A negative g, or 0 * INFINITY, gives a NaN T.
 *   2. Test 5, in addition to the tests 1 to 4 (test 4 with base.value_max_diff * 2^-i stays in force):
 *      fabsf(V_i[q] - V_i[p]) <= T, on the same difference as test 4.  A NaN T rejects every tap but the centre; the pixel
 *      is then kept.
 *   3. Sums.  Beside num and den: num2 = num2 + (w * w) * Var_i[q] from +0, over the accepted taps in visiting order (w * w is
 *      exact; the centre contributes like any accepted tap).
 *   4. Store.  An invalid pixel, or one where only the centre was accepted (den == 9/64), keeps the bits of both V_i[p] and
 *      Var_i[p].  Otherwise V_{i+1}[p] = num / den and Var_{i+1}[p] = num2 / (den * den) (den * den is exact: den is a
 *      multiple of 1/256 not above 1); both divisions correctly rounded, a NaN quotient stored as the quiet NaN 0x7FC00000.
 * The outputs are V_passes and Var_passes.
 * What follows exactly: with value_eps = +INFINITY, a finite sigma_value and a variance plane of finite non-negative values,
 * T is +INFINITY everywhere and out_value has rt_filter_plane's bits; a region of valid pixels with value 1.0f (or 0.0f) and
 * variance +0 keeps both at the default value_eps = 0, because test 5 accepts a difference of 0 (num == den, num2 == 0);
 * normal_min_dot = 2 with unit normals returns both inputs bit for bit.
 * Scope: Var is used as SVGF uses its temporally integrated variance.  With a history of one frame rt_accumulate_plane's
 * out_variance is 0, so at value_eps = 0 the filter only averages equal values there; SVGF's spatial variance estimate for
 * short histories is not built.                                                                                            */
typedef struct rt_filter_variance_params {   /* 32 bytes */
  rt_filter_params base;      /* ranges and checks of rt_filter_params, unchanged                */
  float sigma_value;          /* >= 0 or +INFINITY, not NaN                                      */
  float value_eps;            /* >= 0 or +INFINITY, not NaN                                      */
} rt_filter_variance_params;
/* base = rt_filter_params_default's; sigma_value 4 (SVGF's); value_eps 0.  Stated, not tuned on images.                     */
void rt_filter_variance_params_default(rt_filter_variance_params* params, int32_t width, int32_t height);
/* out_variance is nullable.  out_value may be value and out_variance may be variance (in place); any other overlap of the
 * planes is the caller's error.  The checks are rt_filter_plane's, with the fields of base under their own names, sigma_value
 * and value_eps under theirs, "NULL plane" for value, variance, the guides and out_value, and the 16-byte alignment of the
 * device guides; all of them run before the context is looked at.  Ordering is the filter family's: a variance call and a
 * plain call wait for each other (they share the scratch), nothing else waits for them but rt_destroy.  The scratch is 52
 * bytes per pixel (the guides 32, two value planes 8, two variance planes 8, the thresholds 4), kept and grown like
 * rt_filter_plane's; a context that only ever calls rt_filter_plane allocates its 40.  UOB_RT_FILTER_FORM=direct applies.
 * rt_debug_filter_stats after a variance call: out[2] counts the taps that passed all five tests, and out[5] the taps that
 * passed tests 1 to 4 and failed test 5, over valid centres and passes (0 after a plain rt_filter_plane call).               */
int rt_filter_plane_variance(rt_ctx* ctx, const rt_filter_variance_params* params, const float* value, const float* variance,
                             const float* position4, const float* normal4, float* out_value, float* out_variance);
int rt_filter_plane_variance_device(rt_ctx* ctx, const rt_filter_variance_params* params, const void* d_value,
                                    const void* d_variance, const void* d_position4, const void* d_normal4, void* d_out_value,
                                    void* d_out_variance, void* hip_stream);
/* The same filter on the host (CPU only, no context): the statement the device kernels are pinned against.  Same checks. */
int rt_filter_plane_variance_host(const rt_filter_variance_params* params, const float* value, const float* variance,
                                  const float* position4, const float* normal4, float* out_value, float* out_variance);

/* ---- temporal reprojection of per-pixel planes (rt_accumulate.hip) ------------------------------------
 * Carries a per-pixel estimate from one view to the next: last view's history is gathered at the place where this view's
 * surface point was seen then, under the AOV planes as guides, and the new sample is blended in.  Per pixel the history
 * keeps the first two moments and a history length.  It reads no scene data.  With binary acceptance tests and a fixed
 * operation order it is a pure FP32 function of its inputs; every implementation (the device kernel,
 * rt_accumulate_plane_host) gives the same bits.
 * Scope: the scene is assumed static between the two views.  Camera and light may move; geometry that moved fails the
 * plane or prim test and restarts its history; rt_accumulate_plane_moving below takes the place where a posed or skinned
 * point was (rt_motion_planes) and carries its history along.
 * Planes of `height` rows x `width` pixels, row-major, of the CURRENT view:
 *   value      float32 [h][w]      this view's sample of the estimate;
 *   position4  float32 [h][w][4]   the guides, in the layouts of rt_render_aov's position4 / normal4 planes.  A pixel is
 *   normal4    float32 [h][w][4]   VALID iff position4.w > 0 (a NaN is invalid);
 *   prim       int32   [h][w]      rt_render_aov's prim plane, or NULL: then no tap is tested for its primitive;
 *   prev       rt_history_texel [h][w]   the history the previous call wrote as `next`, or NULL (first frame);
 * and the outputs
 *   next       rt_history_texel [h][w]   required, not the same pointer as prev; any other overlap is the caller's error;
 *   out_mean, out_variance   float32 [h][w], each may be NULL.
 * All arithmetic is FP32 without contraction, in exactly this order, for every pixel p = (x, y), with P / N the xyz of its
 * guides and rot = prev_rot, W = width, H = height:
 *   1. p not valid: mean = value (its bits), m2 = value * value, count = 0.
 *   2. Projection into the previous view (only when prev != NULL): d = P - prev_cam component-wise;
 *      q_j = (d.x*rot[j] + d.y*rot[4+j]) + d.z*rot[8+j] for j = 0, 1, 2 (the columns of rot: R^T d, which inverts the
 *      frame's R * (bx, by*sy, focal) for a rotation matrix); fx = (q0 * prev_focal_px) / q2 + 0.5f * (float)W and
 *      fy = (q1 * prev_focal_px) / q2 + 0.5f * (float)H, the divisions correctly rounded.  The pixel has a CANDIDATE iff
 *      q2 > 0 && fx >= -1 && fx < (float)W && fy >= -1 && fy < (float)H; a NaN fails every comparison.  This inverts sample
 *      0's primary ray (local x = x*aa_x - W*aa_x/2, local y*sy = (y - H/2)*aa_x at focal = prev_focal_px * aa_x), so the
 *      guides of sample 0 of a still view reproject onto integer pixel coordinates up to rounding.
 *   3. Taps: x0 = floorf(fx), y0 = floorf(fy), ax = fx - x0, ay = fy - y0 (both exact).  The four taps (x0+i, y0+j) are
 *      visited with j outer and i inner, both ascending; wt = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay).  A tap with
 *      record r is ACCEPTED iff it lies inside the plane, wt > 0, r.count > 0, prim == NULL || r.prim == prim[p],
 *      (N.x*r.normal.x + N.y*r.normal.y) + N.z*r.normal.z >= normal_min_dot, and with e = r.position - P component-wise
 *      fabsf((N.x*e.x + N.y*e.y) + N.z*e.z) <= plane_eps.  Over the accepted taps in visiting order:
 *      num = num + wt * r.mean, num2 = num2 + wt * r.m2, den = den + wt, all from +0; cmin = the least r.count (exact).
 *   4. prev == NULL, no candidate or no accepted tap: mean = value (its bits), m2 = value * value, count = 1.
 *   5. Otherwise mp = num / den and sp = num2 / den, correctly rounded; n = min(cmin, (float)(max_history - 1)) + 1;
 *      a = 1.0f / n; mean = mp + a * (value - mp); m2 = sp + a * (value * value - sp); count = n.
 *   6. A NaN among the computed results — every m2, and the mean of step 5 — is stored as the quiet NaN 0x7FC00000 (the
 *      sign of a generated NaN differs between x86 and the GPU; the filter has the same rule).  The mean of steps 1 and 4
 *      is a copy and keeps the value's bits, a NaN's payload included.
 *   7. next[p] = (P, mean, N, m2, count, prim[p] or -1, 0, 0): the guides are copied also for an invalid pixel;
 *      out_mean[p] = mean; out_variance[p] = t > 0 ? t : 0 with t = m2 - mean * mean, so a NaN t gives 0.
 * What follows exactly: a region whose values are all 1.0f (or all 0.0f) keeps them for as long as it finds history, since
 * num == den (num == 0); normal_min_dot = 2 with unit normals rejects all history, so every valid pixel is a first frame;
 * count is always an integer value when the history's counts are (0 .. max_history); the variance is never negative or NaN. */
typedef struct rt_history_texel {      /* 48 bytes, 16-byte aligned in device memory */
  float position[3]; float mean;       /* the pixel's guide position | accumulated first moment   */
  float normal[3];   float m2;         /* the pixel's guide normal   | accumulated second moment  */
  float count;                         /* history length, an integer value 0 .. max_history; 0 = no history (invalid pixel) */
  int32_t prim;                        /* the pixel's primitive id (-1 when the call got no prim plane) */
  float pad[2];                        /* written as 0 */
} rt_history_texel;

typedef struct rt_accumulate_params {
  int32_t width, height;       /* >= 1; width * height <= 2^31                                            */
  float   prev_rot[12];        /* the PREVIOUS view: rt_render's rot / cam, and its focal divided by aa_x  */
  float   prev_cam[3];         /*   (focal in pixels); all finite, prev_focal_px > 0                       */
  float   prev_focal_px;
  float   normal_min_dot;      /* not NaN                                                                  */
  float   plane_eps;           /* >= 0, not NaN                                                            */
  int32_t max_history;         /* 1 .. 65536: the blend factor never falls below 1 / max_history           */
} rt_accumulate_params;        /* 84 bytes */
/* Identity prev_rot, zero prev_cam, prev_focal_px = width, normal_min_dot 0.9, plane_eps 0.01, max_history 32: defaults for
 * a scene of the Cornell box's size.  They are stated, not tuned on images.                                              */
void rt_accumulate_params_default(rt_accumulate_params* params, int32_t width, int32_t height);
/* A NULL ctx, params or required plane (value, position4, normal4, next), any parameter outside the ranges above, a view
 * that is not finite, and next == prev are RT_E_INVALID with a message that names the field or argument, before the
 * context is looked at and before any device work.  Ordering: an accumulate call is no reader of the scene — it does not
 * wait for updates, frames, passes, readers or filter calls, and they do not wait for it; it waits only for the context's
 * previous accumulate call (they share the counters and the staging), and rt_destroy waits for it.  Ordering with whatever
 * produces its input planes, the history included, is the caller's stream.  A multi-device context runs it on devices[0].
 * rt_accumulate_plane: host arrays, blocking (staged through device memory the context keeps and only grows).
 * rt_accumulate_plane_device: planes in device memory on the context's device, d_position4 / d_normal4 / d_prev / d_next
 * 16-byte aligned, enqueued on hip_stream (NULL = default stream) after the caller's earlier work; returns without
 * synchronising, and no stage waits for the host.  It needs no scratch: the history buffers are the caller's.  A context
 * that never accumulates allocates nothing for the family.                                                               */
int rt_accumulate_plane(rt_ctx* ctx, const rt_accumulate_params* params, const float* value, const float* position4,
                        const float* normal4, const int32_t* prim, const rt_history_texel* prev, rt_history_texel* next,
                        float* out_mean, float* out_variance);
int rt_accumulate_plane_device(rt_ctx* ctx, const rt_accumulate_params* params, const void* d_value, const void* d_position4,
                               const void* d_normal4, const void* d_prim, const void* d_prev, void* d_next, void* d_out_mean,
                               void* d_out_variance, void* hip_stream);
/* Diagnostic: work counters of the context's most recent accumulate call (synchronises it; zeros before the first).  out[0]
 * pixels, out[1] valid pixels, out[2] valid pixels that found history (at least one accepted tap), out[3] accepted taps,
 * out[4] valid pixels without a candidate (behind the previous camera or outside its frame), out[5..7] 0.  A call without
 * prev makes no projection: out[2..4] are 0.                                                                             */
int rt_debug_accumulate_stats(rt_ctx* ctx, uint64_t out[8]);
/* The same function on the host (CPU only, no context): the statement the device kernel is pinned against.  Same checks. */
int rt_accumulate_plane_host(const rt_accumulate_params* params, const float* value, const float* position4,
                             const float* normal4, const int32_t* prim, const rt_history_texel* prev, rt_history_texel* next,
                             float* out_mean, float* out_variance);

/* ---- motion planes: where posed and skinned geometry was in the previous view (rt_motion.hip) ----------
 * rt_accumulate_plane assumes a static scene.  These entries carry the history across geometry that rt_pose_objects*,
 * rt_pose_skin* or rt_update_scene* moved: the context keeps the scene as the previous view saw it (the SNAPSHOT), a motion
 * call says where each pixel's surface point was in that scene, and rt_accumulate_plane_moving reprojects with that point
 * while it stores the current guides.
 * Scope: triangles.  Sphere motion is out of scope: a sphere element is copied, so a moved sphere (rt_update_spheres) fails
 * the plane test and restarts, as it does with rt_accumulate_plane.  The motion planes are 64 bytes per pixel of
 * intermediate data; a kernel that fuses the motion and the accumulate steps is not built.
 *
 * The snapshot.  rt_motion_snapshot copies the context's live scene, in the caller's original triangle order — vertices
 * [3n] float4 and normals [n] float4 — device to device on hip_stream (NULL = default stream) into buffers the context owns,
 * and records n; it returns without synchronising.  The buffers are sized by the scene, only grow, and are freed by
 * rt_motion_release and rt_destroy; a context that never snapshots allocates nothing.  The caller takes the snapshot after the
 * frame or AOV pass of view k and before the pose or update that makes view k+1.  Nothing in the scene edits changes: an
 * rt_replace_scene* to another triangle count leaves a snapshot whose count no longer matches, and motion calls are
 * refused until the next snapshot.  rt_debug_motion_info: the snapshot's triangle count, 0 without one.
 * Ordering: snapshots and motion calls are one family of readers of the scene.  They wait for the context's pending device
 * edit and for the family's previous call; scene edits wait for them; frames and AOV passes do not wait for them and they do
 * not wait for frames; rt_destroy waits for them.  A multi-device context answers on devices[0].                          */
int rt_motion_snapshot(rt_ctx* ctx, void* hip_stream);
int rt_motion_release(rt_ctx* ctx);
int rt_debug_motion_info(rt_ctx* ctx, int32_t* snapshot_triangles);
/* The motion planes.  Element-wise over `count` elements (no width or height) of rt_render_aov's planes, one sample per
 * pixel or all samples:
 *   prim       int32   [count]      position4, normal4   float32 [count][4]
 * and the outputs out_prev_position4, out_prev_normal4 float32 [count][4], both required.  A pure FP32 function without
 * contraction in exactly this order; every implementation (the device kernel, rt_motion_planes_host) gives the same bits.
 * For element k with P the xyz of position4, n the scene's triangle count, a, b, c the vertices of triangle prim[k] in the
 * live scene and a', b', c' those in the snapshot:
 *   1. INVALID iff position4.w > 0 is false (a NaN is invalid) or prim[k] is outside [-2, n): both outputs are all-zero
 *      (w = 0): no place in the previous scene.
 *   2. prim[k] == -1 (miss-coded but valid) or -2 (a sphere): both outputs are the input planes' bits, all four words.
 *   3. UNMOVED triangle — all nine coordinates compare == with the snapshot's: both outputs are the input planes' bits.  So an
 *      unmoved scene yields its inputs, and accumulation with them equals accumulation without them.
 *   4. MOVED triangle, component-wise: e1 = b - a, e2 = c - a, d = P - a; dot products as (x*x + y*y) + z*z:
 *      d11 = e1.e1, d12 = e1.e2, d22 = e2.e2, p1 = d.e1, p2 = d.e2; den = d11*d22 - d12*d12;
 *      u = (d22*p1 - d12*p2) / den and v = (d11*p2 - d12*p1) / den, the divisions correctly rounded; e1' = b' - a',
 *      e2' = c' - a'; out_prev_position4 = ((a'_c + u*e1'_c) + v*e2'_c for c = x, y, z; 1), a NaN component stored as the quiet
 *      NaN 0x7FC00000 (the filter's and the accumulate's rule; it fails every comparison downstream);
 *      out_prev_normal4 = (the xyz bits of the snapshot's normal of the triangle; 0).
 * Accuracy of step 4 over random rigid moves: the point stays on the previous triangle's plane to about 1.5e-7 for every
 * triangle shape; inside the plane the error is about 3e-7 for well-shaped unit triangles and grows with the aspect ratio
 * (3e-4 at 1:100, 1.7e-2 at 1:1000).  A degenerate triangle (den == 0) gives infinities or the quiet NaN.
 * A NULL ctx or plane and count outside [0, 2^31] are RT_E_INVALID before the context is looked at; so are, after that, a
 * context without a snapshot and one whose snapshot count differs from its current n (the message gives both counts).
 * count == 0 is a no-op.  rt_motion_planes: host arrays, blocking (staged through device memory the context keeps and only
 * grows).  rt_motion_planes_device: planes in device memory on the context's device, the four float4 planes 16-byte
 * aligned, enqueued on hip_stream after the caller's earlier work; returns without synchronising.                          */
int rt_motion_planes(rt_ctx* ctx, const int32_t* prim, const float* position4, const float* normal4, int64_t count,
                     float* out_prev_position4, float* out_prev_normal4);
int rt_motion_planes_device(rt_ctx* ctx, const void* d_prim, const void* d_position4, const void* d_normal4, int64_t count,
                            void* d_out_prev_position4, void* d_out_prev_normal4, void* hip_stream);
/* The same function on the host (CPU only, no context) over a live scene and a previous one of n triangles each, in the
 * layouts of rt_init: the statement the device kernel is pinned against.  Same checks; n >= 0.                             */
int rt_motion_planes_host(const float* vertices4_now, const float* vertices4_then, const float* normals4_then, int32_t n,
                          const int32_t* prim, const float* position4, const float* normal4, int64_t count,
                          float* out_prev_position4, float* out_prev_normal4);
/* Diagnostic: work counters of the context's most recent motion call (synchronises it; zeros before the first).  out[0]
 * elements, out[1] valid elements, out[2] carried through a moved triangle, out[3] on an unmoved triangle, out[4] sphere or
 * miss copies, out[5] valid w but prim out of range, out[6..7] 0.                                                          */
int rt_debug_motion_stats(rt_ctx* ctx, uint64_t out[8]);
/* rt_accumulate_plane with reprojection guides: exactly rt_accumulate_plane's definition with one difference in its steps 2
 * and 3 — the projection, the normal test and the plane test use Pr / Nr, the xyz of
 *   reproj_position4, reproj_normal4   float32 [h][w][4]   (rt_motion_planes' outputs for the view's guides),
 * in place of P / N; a valid pixel whose reproj_position4.w > 0 is false has no candidate (counted in out[4] of
 * rt_debug_accumulate_stats).  The prim test keeps comparing r.prim with prim[p] — triangle indices survive a pose — and
 * step 7 still stores the current P, N and prim.  Both reprojection planes NULL give rt_accumulate_plane bit for bit; one
 * NULL and one set is RT_E_INVALID; in the device entry both are 16-byte aligned.  Checks, ordering, staging and counters
 * are the accumulate family's.                                                                                           */
int rt_accumulate_plane_moving(rt_ctx* ctx, const rt_accumulate_params* params, const float* value, const float* position4,
                               const float* normal4, const int32_t* prim, const float* reproj_position4,
                               const float* reproj_normal4, const rt_history_texel* prev, rt_history_texel* next,
                               float* out_mean, float* out_variance);
int rt_accumulate_plane_moving_device(rt_ctx* ctx, const rt_accumulate_params* params, const void* d_value,
                                      const void* d_position4, const void* d_normal4, const void* d_prim,
                                      const void* d_reproj_position4, const void* d_reproj_normal4, const void* d_prev,
                                      void* d_next, void* d_out_mean, void* d_out_variance, void* hip_stream);
int rt_accumulate_plane_moving_host(const rt_accumulate_params* params, const float* value, const float* position4,
                                    const float* normal4, const int32_t* prim, const float* reproj_position4,
                                    const float* reproj_normal4, const rt_history_texel* prev, rt_history_texel* next,
                                    float* out_mean, float* out_variance);

/* Diagnostic, mesh kernel (n > 64): the cost of every 16x16-pixel block of the most recent frame in s_memtime ticks
 * (shader cycles) — the scheduling state "last frame's expensive blocks first" is built from it.  Row-major over
 * ceil(owned_rows/16) x ceil(width/16) blocks; writes min(count, cap) values, returns the block count, or
 * RT_E_UNSUPPORTED when the context keeps no such state (n <= 64, RT_FLAG_PLAIN_ORDER, generic kernel).          */
int rt_debug_block_costs(rt_ctx* ctx, uint32_t* out, int32_t cap);

/* Diagnostic, mesh kernel (n > 64): the most recent frame's shadow-ray tile masks — for every world cell (x fastest,
 * G x G x G cells) `words` 64-bit words, bit t = "a shadow ray that starts in this cell may hit a triangle of tile t" (tiles in
 * the kernel's own order; a cell no surface point can start from reads 0).  Writes min(count, cap) words, returns the word
 * count G^3 * words and stores G and words, or RT_E_UNSUPPORTED when the context builds no tile masks.                       */
int rt_debug_world_masks(rt_ctx* ctx, uint64_t* out, int64_t cap, int32_t* grid, int32_t* words);

/* Diagnostic, mesh kernel (n > 64): the tiled order and the per-tile data the kernel uses.  orig[j] = original index of the
 * triangle at tiled position j (n entries); tiles = 12 floats per tile (rt_device.h FrameParams::tile_box: box lo.xyz | eta,
 * box hi.xyz | emax, normal-cone axis | chi).  cap_tiles = 0 asks for the tile count only.  Returns the tile count, or
 * RT_E_UNSUPPORTED when the context keeps no tiled copy (n <= 64, RT_FLAG_GENERIC_KERNEL).                              */
int rt_debug_tile_data(rt_ctx* ctx, int32_t* orig, float* tiles, int32_t cap_tiles);

/* Diagnostic: the scene the context holds after its latest edit (rt_update_scene*, rt_replace_scene*, rt_pose_objects*,
 * rt_pose_skin*), read back from the device; a pending device edit is waited for.  Every output is nullable (NULL: not copied):
 *   vertices4 [3n][4], normals4 [n][4], colors4 [n][4]         the scene in the caller's original order, rt_init's layout;
 *   vertices4_m [3n][4], normals4_m [n][4], colors4_m [n][4]   the mesh kernel's tiled copy: entry j is the original
 *                                                              triangle orig[j] of rt_debug_tile_data;
 *   n_shadow                    the triangles that cast shadows (colour w != -1), as the scene's check counted them;
 *   vbox_lo[3], vbox_hi[3]      the vertices' box as the scene's check reduced it.  Only a context with tile masks
 *                               (n > 1024, no RT_FLAG_NO_TILE_BINS / NO_CULL / GENERIC_KERNEL) keeps it; others give zeros.
 * cap_triangles = the triangles every non-NULL array has room for; 0 asks for the count only.  Returns the triangle
 * count n; RT_E_INVALID for a NULL ctx, a negative capacity and 0 < cap_triangles < n; RT_E_UNSUPPORTED when a tiled
 * array is asked of a context that keeps no tiled copy (n <= 64, RT_FLAG_GENERIC_KERNEL).  A multi-device context
 * answers for devices[0].                                                                                              */
int rt_debug_scene_data(rt_ctx* ctx, float* vertices4, float* normals4, float* colors4, float* vertices4_m,
                        float* normals4_m, float* colors4_m, int32_t* n_shadow, float vbox_lo[3], float vbox_hi[3],
                        int32_t cap_triangles);

/* Optional: let the device write the frame STRAIGHT into the caller's host framebuffer (screen->buffer,
 * SDLauxiliary.h:105) instead of rendering into device memory and copying 4 bytes per pixel back after the kernel
 * (clEnqueueReadBuffer, skeleton.cpp:179-180): the pixels cross PCIe while the frame is still being rendered.
 * rt_register_output pins and maps `bytes` bytes at `host` until rt_unregister_output / rt_destroy; every later
 * rt_render of this context whose out_argb range lies inside a registered range (and whose out_rgb_f32 is NULL) takes
 * the direct path.  Same pixels, same blocking semantics.  The caller must not free the memory while it is registered.
 * One range per context.  In a multi-device context every device writes its bands into the range over its own PCIe
 * link (RT_FLAG_STAGED_GATHER keeps the copy engines).                                                             */
int rt_register_output(rt_ctx* ctx, void* host, size_t bytes);
int rt_unregister_output(rt_ctx* ctx);

/* Diagnostic, wave kernel (n <= 64), contexts created with UOB_RT_TIMELINE=1 in the environment: how the persistent
 * waves of the most recent frame spent the kernel's duration, from the 100 MHz s_memrealtime clock.
 *   out[0] waves   out[1] first wave start   out[2] last wave end   out[3] sum of starts   out[4] sum of ends
 *   out[5] jobs done by all waves   out[6] most jobs done by one wave   out[7] length of the expensive-job list the frame started from
 * (start = a wave's first request for a job, end = its exit; mean idle tail = out[2] - out[4]/out[0]).
 * RT_E_UNSUPPORTED when the context was not created with the knob set or its last frame ran on another kernel. */
int rt_debug_wave_timeline(rt_ctx* ctx, uint64_t out[8]);

/* Diagnostic, wave kernel: the tile seeds of the most recent frame (DESIGN.md 4.1 "tile seeds"; devices[0]'s of a
 * multi-device context).  The frame is cut into tiles of dims[2] rows x one job's pixels; before a frame whose kernel
 * takes the seed a pre-pass leaves one 64-byte record per tile, indexed [global row / dims[2]][job column]:
 *   float D0[3], ed;  uint64 K, Kh, Kp;  int32 h;  uint32 flags (1: primary part valid, 2: shadow part valid);  16 bytes unused
 *   dims[0] tile rows   dims[1] tiles per row (jobs per row)   dims[2] rows per tile — all 0 when the last frame took no
 *   seed (UOB_RT_NO_SEED=1, another kernel or instantiation, no frame yet): then nothing is copied and the counters are 0
 *   counters[0] tiles with a valid primary part   counters[1] tiles with a valid shadow part
 *   counters[2], counters[3] jobs of this context's rows that started from one (every job reads its tile's record)
 * Copies min(tiles, cap) records to `records` (may be NULL with cap 0).  Waits for the context's last frame.
 * This is the STRICT view of the table: a primary part counts where the tile's bound leaves one triangle and no sphere, a
 * shadow part where level 1 over such a tile has nothing to do; the fields of a part that is not strict read as unset.  */
int rt_debug_wave_seeds(rt_ctx* ctx, void* records, int64_t cap, int32_t dims[3], uint64_t counters[4]);

/* The same table as the draw kernel reads it (records, cap, dims as above).  flags: 1, 2 the strict bits above;
 *   4  primary part: Kp holds every triangle a primary ray of the tile can hit   8  ... and a sphere may be touched
 *   16 shadow part: D0, ed, K, Kh, h are level 1's outcome around the point the tile's centre ray hits on triangle h
 *   32 ... with a sphere candidate   64 ... blocked (one caster shadows every ray of the set)
 * What is kept: UOB_RT_SEED_KP (most triangles of a primary part), UOB_RT_SEED_CASTERS (most casters off h's plane, Kh, of
 * a shadow part), UOB_RT_SEED_SPH (0: no shadow part with a sphere candidate); a blocked shadow part is always kept.
 *   counters[2 q], counters[2 q + 1]: tiles, and jobs of this context's rows, whose record has   q = 0 a primary part
 *   1 a shadow part   2 a shadow part with Kh != 0   3 a shadow part with a sphere candidate   4 a blocked shadow part  */
int rt_debug_wave_seeds_wide(rt_ctx* ctx, void* records, int64_t cap, int32_t dims[3], uint64_t counters[10]);

/* Diagnostic, several devices in one context (rt_config.devices): the copies that carry device k's packed bands
 * (bands k, k+N, ... of device_band_rows rows, owned rows packed top to bottom in its stripe) to image order in a
 * destination frame of `width` x `height` elements of elem_bytes — exactly what rt_render / rt_render_device enqueue
 * for a device that does not write the destination itself.  Pure arithmetic, no device needed: the cross-device branches
 * cannot run on a one-GPU machine, so tests check and replay the plan on the CPU (tests/test_band_copy_plan.py).
 *   dev_to_dev   : 0 = into host memory (rt_render), 1 = into the root device's memory (rt_render_device)
 *   peer_ok      : the source device may copy 2-D into the root's memory directly (hipDeviceEnablePeerAccess succeeded)
 *   same_device  : the source device IS the root device
 * Writes min(count, cap) entries, returns the count (or a negative RT_E_* code).  Offsets and pitches are in bytes.     */
enum { RT_COPY_2D = 0,      /* hipMemcpy2DAsync: `rows` rows of width_bytes, source pitch src_pitch, destination pitch dst_pitch */
       RT_COPY_PEER = 1,    /* hipMemcpyPeerAsync of width_bytes bytes (no peer mapping, or the ragged last band across devices) */
       RT_COPY_LINEAR = 2   /* hipMemcpyAsync of width_bytes bytes (ragged last band, same device or to the host)          */ };
typedef struct rt_band_copy {
  int32_t op, reserved;
  uint64_t dst_offset, dst_pitch, src_offset, src_pitch, width_bytes, rows;
} rt_band_copy;
int rt_debug_band_copy_plan(int32_t num_devices, int32_t k, int32_t device_band_rows, int32_t width, int32_t height,
                            int32_t elem_bytes, int32_t dev_to_dev, int32_t peer_ok, int32_t same_device,
                            rt_band_copy* out, int32_t cap);

/* On-device self test of the exact-reciprocal building block (rt_math.h rcp_newton): sweeps all 2^32
 * FP32 patterns and compares v_rcp_f32 + 1/2 Newton steps with the correctly rounded 1.0f/x.
 * out[0],out[1] = mismatches (1-step, 2-step) for 2^-100 <= |x| <= 2^100; out[2],out[3] = mismatches for
 * the remaining finite non-zero x; out[4] = examples recorded; out[8..63] = mismatching bit patterns.   */
int rt_selftest_rcp(uint64_t out[64]);

/* On-device self test of normalize()'s building blocks (rt_math.h normalize3): (a) v_rsq_f32 refined once against the
 * correctly rounded sqrtf for every FP32 pattern in [2^-60, 2^60]; (b) the quotient q = fma(fma(-b, a r, a), r, a r) from the
 * exact reciprocal r of b against the correctly rounded a / b for EVERY significand of a and every b_stride-th significand
 * of b (b_stride = 1: all 2^46 pairs, about half a minute; tools/div_check.hip is the same sweep as a program).
 * out[0] mismatches of (a), out[1] mismatches of (b), out[2] pairs checked by (b), out[3] / out[4] a mismatching pattern each. */
int rt_selftest_normalize(uint64_t out[8], uint32_t b_stride);

/* On-device run of the wave and mesh kernels' shade() (rt_wave_common.h: direct_light's running sum of one AA ray, then its
 * colour), one wave of 64 lanes per entry of ns[]: lane l of wave w takes lit / secondary / unshadowed [64 w + l] (lit,
 * secondary: 0 or non-zero; a lit lane's unshadowed lies in 0 .. ns[w]), term[64 w + l] and col[4 (64 w + l) .. + 3], and
 * out[3 (64 w + l) .. + 2] receives its contribution.  ns[w] in 1 .. 4096 is the wave's sample count.  straight_line != 0 runs
 * the instantiation specialised on the sample count where ns[w] is one of 1, 5, 10, 16, 64 (straight-line sums for 64), and the
 * run-time form elsewhere; 0 runs the run-time form everywhere.  All pointers are host memory.                            */
int rt_selftest_shade(int32_t nwaves, const int32_t* ns, const int32_t* lit, const int32_t* secondary, const int32_t* unshadowed,
                      const float* term, const float* col, int32_t straight_line, float* out);

/* On-device run of the wave kernel's all_within() (rt_wave_common.h: "no lane that takes part holds a value above the
 * bound", decided by one compare and a ballot) beside the wave reduction it stands for, one wave of 64 lanes per entry of
 * bound[]: lane l of wave w takes part when in[64 w + l] is non-zero and holds v[64 w + l], which must be >= +0 or NaN;
 * bound[w] must be >= +0 unless some lane of the wave takes part.  out[2 w] receives all_within's answer (0 or 1) and
 * out[2 w + 1] that of  max over the lanes of (in ? v : +0), as bit patterns  <=  bound[w].  All pointers are host memory.  */
int rt_selftest_all_within(int32_t nwaves, const int32_t* in, const float* v, const float* bound, int32_t* out);

/* Releases everything the context holds: it waits for the context's streams, side calls, filter calls and accumulate calls, then frees its device memory,
 * events and streams (and those of every device of a multi-device context), and unregisters a registered output.   */
void rt_destroy(rt_ctx* ctx);

/* Diagnostic: the device objects the library holds at this moment in this process, over all contexts: out[0] device
 * allocations, out[1] their bytes, out[2] events, out[3] streams.  A process without a context reports zeros, and so does one
 * whose every context has been destroyed; calls documented to allocate nothing leave the figures unchanged.  Takes no
 * context and needs no device.                                                                                          */
int rt_debug_live_device_objects(int64_t out[4]);
/* Message of the last failure on the calling thread.  After an RT_OK from rt_init / rt_render_device of a multi-device
 * context it may instead hold a line that starts with "warning:" — a device without peer access to the root device
 * works, through slower copies (band by band), and says so here.                                                      */
const char* rt_last_error(void);
int rt_abi_version(void);

/* ---- scene format (replaces TestModelH.h / Loader.cpp) -------------------------------------- */
/* Triangle AoS exactly as TestModelH.h:14-18: 5 x vec4 = v0, v1, v2, normal, color (80 bytes).      */
typedef struct rt_triangle {
  float v0[4], v1[4], v2[4], normal[4], color[4];
} rt_triangle;

/* LoadTestModel (TestModelH.h:44-219): the 26-triangle Cornell Box.  Writes up to `cap` triangles,
 * returns the triangle count (26) or a negative error.                                               */
int rt_scene_cornell_box(rt_triangle* out, int32_t cap);
/* load_obj (Loader.cpp:11-59): `v x y z` / `f a b c` lines, scale 1.5, negate, translate
 * (-0.4,1.15,-0.7), colour blue (0,0.2,0.4,0.5); normals are those of the un-negated triangle.
 * Returns the triangle count (may exceed cap; only cap are written) or a negative error.             */
int rt_scene_load_obj(const char* path, rt_triangle* out, int32_t cap);
/* load_obj with the constants of Loader.cpp:20,42,48-52 as arguments: color[4] (w = material: >0 diffuse,
 * 0 mirror, <0 glass), scale, and translate[3] applied after the negation (v' = -(scale*v) + translate).
 * NULL color / translate = the reference's (0,0.2,0.4,0.5) / (-0.4,1.15,-0.7); rt_scene_load_obj(path,...) ==
 * rt_scene_load_obj_ex(path, NULL, 1.5f, NULL, ...).                                                          */
int rt_scene_load_obj_ex(const char* path, const float color[4], float scale, const float translate[3],
                         rt_triangle* out, int32_t cap);
/* ComputeNormal (TestModelH.h:26-35): normal = normalize(cross(v2-v0, v1-v0)), w = 1.               */
void rt_triangle_compute_normal(rt_triangle* t);
/* The pose arithmetic on the host (CPU only): the triangles [first, first + count) of tris[0 .. n) get every vertex replaced
 * by v'_r = ((v.x*m_r0 + v.y*m_r1) + v.z*m_r2) + t_r with xform12 = 3 rows x (m_r0, m_r1, m_r2, t_r), FP32 without
 * contraction (w stays), and their normals recomputed by rt_triangle_compute_normal.  A range that is not inside [0, n)
 * changes nothing.                                                                                                   */
void rt_scene_transform(rt_triangle* tris, int32_t n, int32_t first, int32_t count, const float xform12[12]);
/* The skin arithmetic on the host (CPU only), "skinned meshes" above: the triangles [first, first + count) of tris[0 .. n)
 * get every corner replaced by the blend of its four rigid poses (bone_index, weights: [3*count][4], one row per corner;
 * bones12: [nbones][12]; w of the vertex stays), and their normals recomputed by rt_triangle_compute_normal.  A range that is
 * not inside [0, n), or an index >= nbones anywhere in the table, changes nothing.                                      */
void rt_scene_skin(rt_triangle* tris, int32_t n, int32_t first, int32_t count, const uint16_t* bone_index,
                   const float* weights, const float* bones12, int32_t nbones);
/* AoS -> the three packed float4 arrays (skeleton.cpp:474-484).                                      */
void rt_scene_pack(const rt_triangle* tris, int32_t n, float* vertices4, float* normals4, float* colors4);
/* Rotation matrix from yaw/pitch exactly as skeleton.cpp:149-151 (float cos/sin).                    */
void rt_rotation_matrix(float yaw, float pitch, float rot[12]);

#ifdef __cplusplus
}
#endif
#endif /* UOB_RT_H */
