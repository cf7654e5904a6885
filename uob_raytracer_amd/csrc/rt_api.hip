// rt_api.hip — the C-ABI device boundary (include/uob_rt.h) over the gfx950 kernels.
//
// rt_init    replaces opencl_initialise  (Source/skeleton.cpp:366-497): device pick, buffer allocation,
//            one-time blocking upload of the packed scene.
// rt_render  replaces offload_rendering  (Source/skeleton.cpp:146-182): per-frame arguments, the kernel
//            launch that stands where clEnqueueNDRangeKernel(draw) stood (:172), blocking readback (:179).
// There is no CPU fallback: without a HIP device every device entry point fails with RT_E_DEVICE.
//
// Several GPUs in one context (rt_config.num_devices > 1; SURVEY.md 8(b) "Threading", section 5): the context
// owns one child context per listed device, each with its own stream, scene copy and stripe; a frame is launched
// on all of them from the one host thread, and the bands are delivered by the copy engines — straight into the
// caller's host framebuffer over each device's own PCIe link (rt_render), or into the caller's device buffer
// over the direct xGMI link to that device (rt_render_device).  A gather to one root over point-to-point links
// IS N-1 independent peer copies; they occupy no compute unit, so they run beside the next frame's persistent
// grid.  (The one-process-per-GPU flow of bench.py gathers with RCCL through torch.distributed instead.)
//
// Here: the error text, contexts, frames, delivery across devices, output registration and diagnostics.  The scene of a
// context — rt_init's first one (scene_first) and every later edit of it — is rt_scene.hip; the calls beside the frame (ray
// queries, shade and radiance calls, AOV passes) are rt_calls.hip; the context itself is rt_host.h.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "rt_host.h"

namespace uobrt {

static thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
}

KeepError::KeepError() : text(g_last_error) {}
KeepError::~KeepError() { g_last_error = text; }

}  // namespace uobrt

using namespace uobrt;

static int validate_config(const rt_config* c) {
  if (!c) { set_error("rt_config is NULL"); return RT_E_INVALID; }
  if (c->width < 1 || c->height < 1 || c->width > 32767 || c->height > 32767) {
    // the reference casts x,y to short (kernels.cl:427)
    set_error("width/height must be in [1, 32767] (got %dx%d)", c->width, c->height); return RT_E_INVALID;
  }
  if (c->aa_x < 1 || c->aa_y < 1 || c->aa_x > 16 || c->aa_y > 16) { set_error("aa_x/aa_y must be in [1,16]"); return RT_E_INVALID; }
  if (c->shadow_samples < 1 || c->shadow_samples > 4096) { set_error("shadow_samples must be in [1,4096]"); return RT_E_INVALID; }
  if (c->max_bounces < 0 || c->max_bounces > 64) { set_error("max_bounces must be in [0,64]"); return RT_E_INVALID; }
  if (c->num_spheres < 0 || c->num_spheres > RT_MAX_SPHERES) { set_error("num_spheres must be in [0,%d]", RT_MAX_SPHERES); return RT_E_INVALID; }
  if (c->band_count < 1 || c->band_index < 0 || c->band_index >= c->band_count || c->band_rows < 1) {
    set_error("band partition invalid (rows=%d index=%d count=%d)", c->band_rows, c->band_index, c->band_count); return RT_E_INVALID;
  }
  if (!(c->light_spread >= 0.0f) || !(c->light_spread <= kMaxCoordinate)) { set_error("light_spread must be in [0, 2^16]"); return RT_E_INVALID; }
  if (validate_spheres(c->spheres, c->num_spheres) != RT_OK) return RT_E_INVALID;
  if ((double)c->width * c->height > 16777216.0) {
    // global_id = y*W+x is formed in FP32 by the reference (kernels.cl:380): exact only up to 2^24
    set_error("width*height must not exceed 2^24 (the reference's FP32 pixel id)"); return RT_E_INVALID;
  }
  if (c->flags & 1) { set_error("flag bit 0 (the former RT_FLAG_FAST_MATH) is not defined in ABI %d", RT_ABI_VERSION); return RT_E_UNSUPPORTED; }
  if (c->num_devices < 0 || c->num_devices > RT_MAX_DEVICES || c->device_band_rows < 0) {
    set_error("num_devices must be in [0,%d] and device_band_rows >= 0", RT_MAX_DEVICES); return RT_E_INVALID;
  }
  if (c->num_devices > 1 && c->band_count != 1) {
    set_error("several devices in one context need the whole frame (band_count == 1)"); return RT_E_UNSUPPORTED;
  }
  return RT_OK;
}

static Tuning read_tuning(const rt_config& cfg) {
  Tuning t;
  if (const char* e = getenv("UOB_RT_JOB_TASKS")) t.job_tasks = atoi(e);
  if (const char* e = getenv("UOB_RT_HEAVY_FACTOR4")) { const int v = atoi(e); if (v >= 1 && v <= 4096) t.heavy_factor4 = v; }
  t.plain_order = (cfg.flags & RT_FLAG_PLAIN_ORDER) != 0 || getenv("UOB_RT_PLAIN_ORDER") != nullptr;
  t.full_grid = getenv("UOB_RT_FULL_GRID") != nullptr;
  t.no_specialise = getenv("UOB_RT_NO_SPECIALISE") != nullptr;
  if (const char* e = getenv("UOB_RT_HEAVY_DILATE")) t.heavy_dilate = atoi(e) != 0;
  if (const char* e = getenv("UOB_RT_L1_INFLATE")) { const float v = (float)atof(e); if (v >= 1.0f && v <= 64.0f) t.l1_inflate = v; }
  if (const char* e = getenv("UOB_RT_GRID_PER_CU")) { const int v = atoi(e); if (v >= 1 && v <= 8) t.grid_per_cu = v; }
  t.phase_profile = getenv("UOB_RT_PHASE_PROFILE") != nullptr;
  t.timeline = getenv("UOB_RT_TIMELINE") != nullptr;
  if (const char* e = getenv("UOB_RT_MASK_DEBUG")) t.mask_debug = atoi(e);
  if (const char* e = getenv("UOB_RT_TILE_ORDER")) t.tile_morton = !strcmp(e, "morton");
  if (const char* e = getenv("UOB_RT_NO_SEED")) t.no_seed = atoi(e) != 0;
  if (const char* e = getenv("UOB_RT_SEED_ROWS")) { const int v = atoi(e); if (v >= 1 && v <= 64) t.seed_rows = v; }
  if (const char* e = getenv("UOB_RT_SEED_KP")) { const int v = atoi(e); if (v >= 1 && v <= 64) t.seed_kp = v; }
  if (const char* e = getenv("UOB_RT_SEED_CASTERS")) { const int v = atoi(e); if (v >= 0 && v <= 64) t.seed_casters = v; }
  if (const char* e = getenv("UOB_RT_SEED_SPH")) t.seed_sph = atoi(e) != 0;
  if (const char* e = getenv("UOB_RT_MOTION_BLOCKS_X")) { const int v = atoi(e); if (v >= 1 && v <= kMotionBlocksX) t.motion_blocks_x = v; }
  if (const char* e = getenv("UOB_RT_FILTER_FORM")) t.filter_form = !strcmp(e, "direct") ? kFilterFormDirect : kFilterFormBuiltIn;
  return t;
}

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }
const char* rt_last_error(void) { return g_last_error.c_str(); }

void rt_config_default(rt_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof *cfg);
  cfg->width = 1024; cfg->height = 1024;           // skeleton.cpp:32-33
  cfg->aa_x = 2; cfg->aa_y = 2;                    // kernels.cl:12-13
  cfg->shadow_samples = 10; cfg->light_spread = 0.05f;   // kernels.cl:316-317
  cfg->max_bounces = 10;                           // kernels.cl:343
  cfg->num_spheres = 2;                            // kernels.cl:7-10 (third initialiser dropped)
  const rt_sphere glass = {{0.3f, 0.1f, -0.5f}, 0.075f, {0.0f, 0.f, 0.f, -1.0f}};
  const rt_sphere mirror = {{-0.4f, 0.8f, -0.5f}, 0.05f, {0.0f, 0.f, 0.f, 0.0f}};
  cfg->spheres[0] = glass; cfg->spheres[1] = mirror;
  cfg->band_rows = cfg->height; cfg->band_index = 0; cfg->band_count = 1;
  cfg->device = -1; cfg->flags = 0;
  cfg->num_devices = 0; cfg->device_band_rows = 0;
}

int32_t rt_config_owned_rows(const rt_config* c) {
  if (!c || c->band_rows < 1 || c->band_count < 1) return 0;
  int rows = 0;
  for (int y = 0; y < c->height; ++y) rows += ((y / c->band_rows) % c->band_count) == c->band_index;
  return rows;
}

static int init_parent(const rt_config* cfg, const float* vertices4, const float* normals4, const float* colors4,
                       int32_t n, rt_ctx** out_ctx) {
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev < 1) { set_error("no HIP device present"); return RT_E_DEVICE; }
  for (int d = 0; d < cfg->num_devices; ++d)
    if (cfg->devices[d] < 0 || cfg->devices[d] >= ndev) {
      set_error("devices[%d] = %d, but %d HIP device(s) are present", d, cfg->devices[d], ndev); return RT_E_INVALID;
    }
  std::unique_ptr<rt_ctx> p(new (std::nothrow) rt_ctx());   // a failure below deletes it, its children included
  if (!p) { set_error("out of host memory"); return RT_E_NOMEM; }
  std::string downgrade;                     // devices that will copy band by band (reported through rt_last_error)
  p->cfg = *cfg;
  p->device = cfg->devices[0];
  p->n = n; p->cap = n > 0 ? n : 1;
  p->owned_rows = rt_config_owned_rows(cfg);
  const int dbr = cfg->device_band_rows > 0 ? cfg->device_band_rows : 32;
  p->cfg.device_band_rows = dbr;
  for (int d = 0; d < cfg->num_devices; ++d) {
    rt_config kc = *cfg;
    kc.num_devices = 0; kc.device = cfg->devices[d];
    kc.band_rows = dbr; kc.band_index = d; kc.band_count = cfg->num_devices;
    rt_ctx* k = nullptr;
    const int rc = rt_init(&kc, vertices4, normals4, colors4, n, &k);
    if (rc != RT_OK) return rc;
    p->kids.push_back(k);
    if (hipSetDevice(k->device) != hipSuccess || k->ev_done.create(hipEventDisableTiming) != hipSuccess) {
      set_error("event creation failed on device %d", k->device); return RT_E_DEVICE;
    }
    if (k->device != p->device) {           // let the copy engines of this device write the root's memory directly
      int can = 0;
      hipError_t e = hipDeviceCanAccessPeer(&can, k->device, p->device);
      if (e == hipSuccess && can) {
        e = hipDeviceEnablePeerAccess(p->device, 0);
        k->peer_ok = (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled);
      } else {
        k->peer_ok = false;
      }
      (void)hipGetLastError();
      if (!k->peer_ok) {                     // not an error: the bands travel band by band through hipMemcpyPeerAsync — but say so
        char line[160];
        snprintf(line, sizeof line, "%sdevice %d has no peer access to device %d (%s)", downgrade.empty() ? "warning: " : "; ",
                 k->device, p->device, e == hipSuccess ? "hipDeviceCanAccessPeer: no" : hipGetErrorString(e));
        downgrade += line;
      }
    }
  }
  if (hipSetDevice(p->device) != hipSuccess || p->ev_go.create(hipEventDisableTiming) != hipSuccess ||
      p->stream.create() != hipSuccess || p->ev0.create() != hipSuccess || p->ev1.create() != hipSuccess) {
    set_error("stream/event creation failed on device %d", p->device); return RT_E_DEVICE;
  }
  // RT_OK with a "warning: ..." line in rt_last_error(): the context works, through the slower copies
  if (!downgrade.empty()) set_error("%s: their bands are copied band by band (hipMemcpyPeerAsync)", downgrade.c_str());
  *out_ctx = p.release();
  return RT_OK;
}

int rt_init(const rt_config* cfg, const float* vertices4, const float* normals4, const float* colors4,
            int32_t n, rt_ctx** out_ctx) {
  if (!out_ctx) { set_error("out_ctx is NULL"); return RT_E_INVALID; }
  *out_ctx = nullptr;
  int rc = validate_config(cfg);
  if (rc != RT_OK) return rc;
  if (n < 0 || (n > 0 && (!vertices4 || !normals4 || !colors4))) { set_error("scene arrays missing"); return RT_E_INVALID; }
  rc = validate_vertices(vertices4, n);
  if (rc != RT_OK) return rc;
  if (n > kMaxTriangles) { set_error("triangle list of %d exceeds the supported maximum of %d", n, kMaxTriangles); return RT_E_UNSUPPORTED; }
  DeviceGuard guard;
  if (cfg->num_devices > 1) return init_parent(cfg, vertices4, normals4, colors4, n, out_ctx);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev < 1) { set_error("no HIP device present"); return RT_E_DEVICE; }
  std::unique_ptr<rt_ctx> c(new (std::nothrow) rt_ctx());   // a failure below deletes it (declared after the guard)
  if (!c) { set_error("out of host memory"); return RT_E_NOMEM; }
  c->cfg = *cfg;
  c->tune = read_tuning(*cfg);
  if (cfg->num_devices == 1) c->device = cfg->devices[0];
  else if (cfg->device >= 0) c->device = cfg->device;
  else hipGetDevice(&c->device);
  if (hipSetDevice(c->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", c->device); return RT_E_DEVICE; }
  c->owned_rows = rt_config_owned_rows(cfg);
  if (hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || c->cus < 1) c->cus = 256;
  const size_t px = (size_t)(c->owned_rows > 0 ? c->owned_rows : 1) * cfg->width;
  if (c->d_argb.alloc(px) != hipSuccess || c->d_counters.alloc(sizeof(rt_work) / sizeof(unsigned long long)) != hipSuccess ||
      c->d_jobctr.alloc((2 * kJobHeads + 2) * kJobHeadStride) != hipSuccess || c->d_spheres.alloc(RT_MAX_SPHERES) != hipSuccess)
    return alloc_failed();
  {   // wave kernel: lists of last frame's expensive jobs (sized for the smallest job, one 64-ray task)
    const int aa = cfg->aa_x * cfg->aa_y;
    const int pt = (aa >= 1 && aa <= 64) ? 64 / aa : 16;        // smallest job: one task; more than 64 AA samples: 16 pixels
    const size_t jobs_max = (size_t)((cfg->width + pt - 1) / pt) * (size_t)(c->owned_rows > 0 ? c->owned_rows : 1);
    c->heavy_cap = (int)(jobs_max / 3 > 64 ? jobs_max / 3 : 64);
    c->heavy_jobs_max = jobs_max;
  }
  if (c->stream.create() != hipSuccess || c->ev0.create() != hipSuccess || c->ev1.create() != hipSuccess) {
    set_error("stream/event creation failed"); return RT_E_DEVICE;
  }
  rc = upload_spheres(c.get());
  if (rc != RT_OK) return rc;
  // the scene: buffers by n, upload, tiles, n_shadow, scene box, kernel family — the routine every later edit goes through (rt_scene.hip)
  rc = scene_first(c.get(), vertices4, normals4, colors4, n);
  if (rc != RT_OK) return rc;
  *out_ctx = c.release();
  return RT_OK;
}

}  // extern "C"

// fill_params, part 1: the view, the frame's constants and the scene
static void fill_view_and_scene(const rt_ctx* c, const float rot[12], const float cam[3], const float light[3], float focal,
                                FrameParams* P) {
  memcpy(P->rot, rot, 12 * sizeof(float));
  memcpy(P->cam, cam, 3 * sizeof(float));
  memcpy(P->light, light, 3 * sizeof(float));
  P->focal = focal;
  const rt_config& g = c->cfg;
  P->spread = g.light_spread;
  P->W = g.width; P->H = g.height; P->aa_x = g.aa_x; P->aa_y = g.aa_y;
  P->S = g.shadow_samples; P->bounces = g.max_bounces; P->nsph = g.num_spheres; P->n = c->n;
  P->band_rows = g.band_rows; P->band_index = g.band_index; P->band_count = g.band_count;
  P->owned_rows = c->owned_rows;
  P->sy = (float)g.aa_x / (float)g.aa_y;
  {   // frame invariants of the reference's arithmetic (rt_device.h), same FP32 operations as the kernels would perform
    P->half_wx = ((float)g.width * (float)g.aa_x) / 2.0f;
    P->half_hy = ((float)g.height * (float)g.aa_y) / 2.0f;
    P->w_f = (float)g.width;
    P->focal0 = focal + 0.0f;
    P->rzf[0] = rot[2] * P->focal0; P->rzf[1] = rot[6] * P->focal0; P->rzf[2] = rot[10] * P->focal0;
    P->hbox = g.light_spread / 2.f;
    P->light_inf = fmaxf(fmaxf(fabsf(light[0]), fabsf(light[1])), fabsf(light[2]));
    P->band_rows_magic = div_magic_for(g.band_rows);
  }
  {
    const int aa = g.aa_x * g.aa_y;
    P->inv_S = (g.shadow_samples & (g.shadow_samples - 1)) == 0 ? 1.0f / (float)g.shadow_samples : 0.0f;
    P->inv_aa = (aa & (aa - 1)) == 0 ? 1.0f / (float)aa : 0.0f;
  }
  P->n_shadow = c->n_shadow;
  for (int i = 0; i < g.num_spheres; ++i) {
    P->sph[i].cx = g.spheres[i].center[0]; P->sph[i].cy = g.spheres[i].center[1]; P->sph[i].cz = g.spheres[i].center[2];
    P->sph[i].r2 = g.spheres[i].radius_sq;
    memcpy(P->sph[i].col, g.spheres[i].color, 16);
  }
  P->verts = c->d_verts; P->normals = c->d_normals; P->colors = c->d_colors;
  P->sph_dev = c->d_spheres;
  P->records = c->d_records;
  P->mask_debug = c->tune.mask_debug;
  P->job_counter = c->d_jobctr + kJobHeadStride;      // [HeavyState 0 | queue heads | HeavyState 1], one line each
}

// fill_params, part 2: the wave kernel's job layout — a job is a run of job_tasks 64-ray tasks (job_tasks * 64/aa pixels) of one row
static void fill_wave_jobs(const rt_ctx* c, const float rot[12], FrameParams* P) {
  const rt_config& g = c->cfg;
  const int aa = g.aa_x * g.aa_y;
  const bool wave_aa = aa >= 1 && aa <= 64;
  const int big_chunks = aa > 64 ? (aa + 63) / 64 : 0;      // 65..256 AA samples: a pixel is big_chunks tasks (rt_kernel_wave.hip BIGAA)
  // Job size: up to 64 pixels, halved while the queue would hold fewer than ~16 jobs per resident wave (jobs differ
  // 10x in cost, but every hand-out stalls its wave for microseconds; measured with last frame's expensive jobs
  // going first: 4096 and 2048 rows -> 64 px, 1024 and 512 rows -> 32 px), but not below 16 pixels.
  const int pt = wave_aa ? 64 / aa : 64;              // pixels per 64-ray task
  P->aa_magic = wave_aa ? (65536 + aa - 1) / aa : 65536;
  P->aax_magic = (65536 + g.aa_x - 1) / g.aa_x;
  // workgroups the chip holds at once; a rank of a multi-GPU job leaves one slot per CU free (registers and LDS
  // for a workgroup of a collective's kernels), so that the gather of the previous frame can run beside it
  const int per_cu = c->tune.grid_per_cu ? c->tune.grid_per_cu : wave_blocks_per_cu(g.band_count > 1 && !c->tune.full_grid);
  P->wave_blocks = c->cus * per_cu;
  const long waves = (long)P->wave_blocks * 4;
  int jt = wave_aa ? 64 / pt : 1;                      // tasks of a 64-pixel job (aa for the power-of-two grids)
  while (jt > 1 && ((jt + 1) / 2) * pt >= 16 && (long)((g.width + jt * pt - 1) / (jt * pt)) * c->owned_rows < 16 * waves) jt = (jt + 1) / 2;
  // (the knob may not make a job smaller than 16 pixels: div_magic's exactness bound, rt_device.h, is stated for >= 16)
  if (wave_aa && c->tune.job_tasks >= 1 && c->tune.job_tasks * pt <= 64 && (c->tune.job_tasks * pt >= 16 || c->tune.job_tasks >= jt))
    jt = c->tune.job_tasks;
  if (big_chunks) jt = 16 * big_chunks;                      // jobs of 16 pixels
  // job / nseg by one multiply-high (rt_device.h div_magic) is exact while (njobs - 1) * (magic * nseg - 2^32) < 2^32.
  // Every accepted frame with jobs of 16+ pixels satisfies it; a knob that asks for smaller jobs is honoured only as far
  // as the bound still holds (checked here, not assumed): the job is doubled until it does.
  int job_pixels = 0;
  for (;;) {
    job_pixels = big_chunks ? jt / big_chunks : jt * pt;
    P->nseg = (g.width + job_pixels - 1) / job_pixels;
    P->njobs = P->nseg * c->owned_rows;
    P->nseg_magic = div_magic_for(P->nseg);
    if (big_chunks) break;                                     // 16-pixel jobs: within div_magic's bound for every accepted frame
    const uint64_t err = P->nseg_magic ? (uint64_t)P->nseg_magic * (uint64_t)P->nseg - 0x100000000ull : 0ull;
    if ((uint64_t)(P->njobs > 0 ? P->njobs - 1 : 0) * err < 0x100000000ull || 2 * jt * pt > 64) break;
    jt *= 2;
  }
  P->job_tasks = jt;
  P->no_specialise = c->tune.no_specialise ? 1 : 0;
  P->l1_inflate = c->tune.l1_inflate;
  P->job_hx = 0.5f * (float)(job_pixels * g.aa_x - 1);
  P->job_hy = 0.5f * (float)(g.aa_y - 1) * P->sy;
  for (int k = 0; k < 3; ++k)
    P->job_eu[k] = 1.0001f * (fabsf(rot[4 * k]) * P->job_hx + fabsf(rot[4 * k + 1]) * P->job_hy);
}

// fill_params, part 3: the mesh kernel's tile masks and their world grid (a context that builds them: c->d_screen_masks)
static void fill_world_grid(const rt_ctx* c, const float cam[3], const float light[3], FrameParams* P) {
  const rt_config& g = c->cfg;
  P->screen_masks = c->d_screen_masks; P->world_masks = c->d_world_masks; P->world_occ = c->d_world_occ;
  P->nwords = c->nwords; P->scx = c->scx; P->scy = c->scy; P->grid_g = kWorldGrid;
  // World grid: a cube over the scene box, grown so that every shadow-ray start point X + 1e-4 (light - X)
  // of a surface point X in the box (kernels.cl:324) stays inside, rounding included; X itself is computed
  // from the camera (X = cam + t dir, or v0 + u e1 + v e2), so its rounding scales with the camera's and the
  // scene's coordinates.
  float ext = 0.0f, dmax = 0.0f, amax = 0.0f, cmax = 0.0f;
  for (int k = 0; k < 3; ++k) {
    ext = fmaxf(ext, c->box_hi[k] - c->box_lo[k]);
    dmax = fmaxf(dmax, fmaxf(fabsf(light[k] - c->box_lo[k]), fabsf(light[k] - c->box_hi[k])));
    amax = fmaxf(amax, fmaxf(fabsf(c->box_lo[k]), fabsf(c->box_hi[k])));
    cmax = fmaxf(cmax, fabsf(cam[k]));
  }
  float grow = 2e-4f * dmax + 1e-4f * (amax + cmax) + 1e-3f * ext + 1e-30f;
  // hit points on spheres can lie 2e-3 (|ray origin - centre| + R) off the sphere (rt_bin_occupancy): the grid holds them
  for (int i = 0; i < g.num_spheres; ++i) {
    float l2 = 0.0f;
    for (int k = 0; k < 3; ++k) l2 += (cam[k] - g.spheres[i].center[k]) * (cam[k] - g.spheres[i].center[k]);
    const float far = fmaxf(sqrtf(l2), 1.7321f * (ext + 2.0f * grow));
    grow = fmaxf(grow, 2.5e-3f * (far + sqrtf(fmaxf(g.spheres[i].radius_sq, 0.0f))));
  }
  for (int k = 0; k < 3; ++k) P->grid_lo[k] = c->box_lo[k] - grow;
  P->grid_cell = (ext + 2.0f * grow) / (float)kWorldGrid;
  P->grid_inv = 1.0f / P->grid_cell;
}

void uobrt::fill_params(const rt_ctx* c, const float rot[12], const float cam[3], const float light[3], float focal,
                        FrameParams* P) {
  memset(P, 0, sizeof *P);
  fill_view_and_scene(c, rot, cam, light, focal, P);
  fill_wave_jobs(c, rot, P);
  if (c->d_screen_masks) fill_world_grid(c, cam, light, P);
}

// The mesh kernel works on the reordered copy of the scene (rt_scene.hip upload_tiled_scene)
void uobrt::use_tiled_scene(const rt_ctx* c, FrameParams* P) {
  P->verts = c->d_verts_m; P->normals = c->d_normals_m; P->colors = c->d_colors_m;
  P->orig = c->d_orig; P->tile_box = c->d_tile_box;
  P->mesh_blocks = c->cus * mesh_blocks_per_cu();
}

// FrameParams of the scene only, for what looks at no view: identity view, the given light, and the tiled copy when `tiled`
// (the readers of rt_calls.hip pass "the context keeps one"; the brute-force rt_debug_trace_rays reads the original order)
void uobrt::scene_params(const rt_ctx* c, const float light[3], bool tiled, FrameParams* P) {
  const float zero3[3] = {0.f, 0.f, 0.f}, ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  fill_params(c, ident, zero3, light, 1.0f, P);
  if (tiled) use_tiled_scene(c, P);
}

// ---- which kernel renders a frame ----------------------------------------------------------------------------------------
// The ONE statement of it (DESIGN.md 4, table at its head), for launch_frame and rt_count_executed alike; which wave
// instantiation is rt_kernel_wave.hip's (kWaveVariants).  It reads the context's working pointers through P (P.records), as
// scene_select (rt_scene.hip) leaves them: a context made with RT_FLAG_GENERIC_KERNEL has no tiled copy to render from.
enum class Family { wave, mesh, generic };

static bool frame_cull(const rt_ctx* c) { return !(c->cfg.flags & RT_FLAG_NO_CULL); }

static Family frame_family(const rt_ctx* c, const FrameParams& P) {
  if (c->cfg.flags & RT_FLAG_GENERIC_KERNEL) return Family::generic;
  // (more than 64 AA samples per pixel: the wave kernel's chunked instantiation exists with the cull only)
  if (wave_kernel_supports(P) && (frame_cull(c) || P.aa_x * P.aa_y <= 64)) return Family::wave;
  return frame_cull(c) && mesh_kernel_supports(P) ? Family::mesh : Family::generic;
}

// Wave kernel: last frame's expensive jobs first — where jobs are long enough (4+ tasks) for the extra look-up per
// hand-out not to matter (measured: 1024^2 frames with 16-pixel jobs lose 12-18 % to it, larger ones gain 2-8 %)
static void attach_heavy_lists(rt_ctx* c, FrameParams* P) {
  if (!c->d_heavy_flags || P->job_tasks < 4) return;
  const int prev = c->heavy_phase, cur = prev ^ 1;
  unsigned int* const st[2] = {c->d_jobctr, c->d_jobctr + (2 * kJobHeads + 1) * kJobHeadStride};
  P->heavy_prev = c->d_heavy[prev]; P->heavy_prev_state = st[prev];
  P->heavy_new = c->d_heavy[cur]; P->heavy_new_state = st[cur];
  P->heavy_flags = c->d_heavy_flags + (size_t)prev * c->heavy_jobs_max; P->heavy_flags_new = c->d_heavy_flags + (size_t)cur * c->heavy_jobs_max;
  P->heavy_gen = ++c->heavy_gen;
  P->heavy_factor4 = c->tune.heavy_factor4;                      // expensive = more than twice the average job
  P->heavy_cap = P->njobs / 3 < c->heavy_cap ? P->njobs / 3 : c->heavy_cap;
  P->heavy_dilate = c->tune.heavy_dilate ? 1 : 0;
  c->heavy_phase = cur;
}

// Wave kernel, diagnostic (UOB_RT_TIMELINE): the shipped kernel, with its per-wave start / end stamps
static int attach_timeline(rt_ctx* c, hipStream_t stream, FrameParams* P) {
  c->timeline_valid = false;
  if (!c->tune.timeline) return RT_OK;
  const size_t waves = (size_t)P->wave_blocks * 4;
  if (!c->d_timeline) {
    if (c->d_timeline.alloc(waves * 3) != hipSuccess) { set_error("hipMalloc failed (timeline)"); return RT_E_NOMEM; }
    c->timeline_waves = waves;
  }
  if (c->timeline_waves >= waves) {
    HIP_TRY(hipMemsetAsync(c->d_timeline, 0, c->timeline_waves * 3 * sizeof(uint64_t), stream));
    P->counters = reinterpret_cast<unsigned long long*>(c->d_timeline.p);
    c->timeline_valid = true;
  }
  return RT_OK;
}

// Wave kernel, the tile seeds (rt_kernel_wave.hip rt_wave_seed): written from THIS frame's parameters in front of the draw
// kernel on the caller's stream, every frame — view, light, scene and spheres may all have changed since the last one.  The
// table is one more of the buffers a context's frames share: "one frame of a context at a time" orders its writers and
// readers as it orders those of the queue heads and the expensive-job lists.
static int attach_seeds(rt_ctx* c, const float rot[12], FrameParams* P) {
  if (c->tune.no_seed || !wave_takes_seed(*P, frame_cull(c))) return RT_OK;
  const int R = c->tune.seed_rows;
  const int tile_rows = (P->H + R - 1) / R;
  const size_t tiles = (size_t)tile_rows * (size_t)P->nseg;
  if (c->seed_cap < tiles) {
    if (c->d_seed.alloc(tiles) != hipSuccess) return alloc_failed();
    c->seed_cap = tiles;
  }
  P->seed = c->d_seed; P->seed_rows = R; P->seed_tile_rows = tile_rows; P->seed_rows_magic = div_magic_for(R);
  P->seed_hy = 0.5f * (float)(R * P->aa_y - 1) * P->sy;
  for (int k = 0; k < 3; ++k) P->seed_eu[k] = 1.0001f * (fabsf(rot[4 * k]) * P->job_hx + fabsf(rot[4 * k + 1]) * P->seed_hy);
  P->seed_kp_cap = c->tune.seed_kp; P->seed_caster_cap = c->tune.seed_casters; P->seed_keep_sph = c->tune.seed_sph ? 1 : 0;
  c->seed_tile_rows = tile_rows; c->seed_nseg = P->nseg; c->seed_rows = R;
  return RT_OK;
}

// One frame of a single-device context into d_argb (packed rows, or global rows when out_global) on `stream`
static int launch_frame(rt_ctx* c, const float rot[12], const float cam[3], const float light[3], float focal,
                        uint32_t* d_argb, float4* d_rgb, hipStream_t stream, bool out_global = false) {
  if (!c || !rot || !cam || !light) { set_error("NULL argument"); return RT_E_INVALID; }
  for (int k = 0; k < 3; ++k)
    if (!(fabsf(cam[k]) <= kMaxCoordinate) || !(fabsf(light[k]) <= kMaxCoordinate)) {
      set_error("camera / light coordinates must be finite and <= 2^16"); return RT_E_INVALID;
    }
  if (!(fabsf(focal) <= 1.0e9f)) { set_error("focal length must be finite and <= 1e9"); return RT_E_INVALID; }
  for (int k = 0; k < 12; ++k)
    if (!(fabsf(rot[k]) <= 4.0f)) { set_error("rotation matrix entries must be finite and <= 4"); return RT_E_INVALID; }
  if (c->owned_rows == 0) return RT_OK;
  FrameParams P;
  fill_params(c, rot, cam, light, focal, &P);
  P.out_argb = d_argb; P.out_rgb = d_rgb; P.counters = nullptr;
  P.out_global = out_global ? 1 : 0;
  HIP_TRY(hipSetDevice(c->device));
  // one frame of a context at a time: the queue heads, the expensive-job lists and the tile masks are shared
  if (c->timed && stream != c->last_stream) HIP_TRY(hipStreamWaitEvent(stream, c->ev1, 0));
  HIP_TRY(wait_aov(c, stream));
  HIP_TRY(wait_scene(c, stream));          // before ev0: rt_last_kernel_ms times the frame's kernels only
  HIP_TRY(hipEventRecord(c->ev0, stream));
  c->seed_tile_rows = 0;                      // (set again by a frame that takes the seed)
  const Family family = frame_family(c, P);
  if (family == Family::wave) {
    attach_heavy_lists(c, &P);
    int rc = attach_timeline(c, stream, &P);
    if (rc == RT_OK) rc = attach_seeds(c, rot, &P);
    if (rc != RT_OK) return rc;
    launch_wave(P, frame_cull(c), false, false, stream);
  } else if (family == Family::mesh) {
    use_tiled_scene(c, &P);
    if (c->d_mesh_cost) {                   // last frame's expensive blocks first; this frame's costs make the next order
      P.mesh_order = c->mesh_order_valid ? c->d_mesh_order : nullptr;
      P.mesh_cost = c->d_mesh_cost; P.mesh_order_out = c->d_mesh_order;
      P.mesh_queue_len = c->d_mesh_order + 4 * (size_t)((c->cfg.width + 15) / 16) * (size_t)((c->owned_rows + 15) / 16);
      c->mesh_order_valid = true;
    }
    launch_stage_records(P, stream);        // per frame: the records hold camera-dependent terms
    launch_mesh(P, false, false, stream, c->aux_stream, c->ev_fork, c->ev_join);
  } else {
    launch_generic(P, false, stream);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev1, stream));
  c->timed = true;
  c->last_stream = stream;
  return RT_OK;
}

// ---- several devices --------------------------------------------------------------------------------------
// Child k of a parent with N children owns the bands k, k+N, ... of `dbr` rows; its stripe holds them packed.
// band_copy_plan lists the copies that put them into image order at the destination (row pitch W elements of `elem`
// bytes): one 2-D copy whose "rows" are whole bands, plus the ragged last band if this child owns it.  The plan is
// pure arithmetic (no HIP call): rt_debug_band_copy_plan exposes it so that a CPU test can check every offset and pitch
// and replay it with memcpy — the cross-device branches cannot run on a one-GPU box.
static int band_copy_plan(int N, int k, int dbr, int W, int owned_rows, size_t elem, bool dev_to_dev, bool peer_ok,
                          bool same_device, rt_band_copy* out, int cap) {
  const size_t band_bytes = (size_t)dbr * W * elem;
  const int full = owned_rows / dbr, rem = owned_rows % dbr;
  const size_t d0 = (size_t)k * band_bytes;
  int cnt = 0;
  auto emit = [&](int op, size_t doff, size_t dpitch, size_t soff, size_t spitch, size_t width, size_t rows) {
    if (cnt < cap && out) {
      rt_band_copy& c = out[cnt];
      c.op = op; c.reserved = 0; c.dst_offset = doff; c.dst_pitch = dpitch; c.src_offset = soff; c.src_pitch = spitch;
      c.width_bytes = width; c.rows = rows;
    }
    ++cnt;
  };
  if (full > 0) {
    if (!dev_to_dev || peer_ok) {
      emit(RT_COPY_2D, d0, (size_t)N * band_bytes, 0, band_bytes, band_bytes, (size_t)full);
    } else {                                   // no peer mapping: band by band through the runtime
      for (int b = 0; b < full; ++b)
        emit(RT_COPY_PEER, d0 + (size_t)b * N * band_bytes, 0, (size_t)b * band_bytes, 0, band_bytes, 1);
    }
  }
  if (rem > 0) {
    const size_t bytes = (size_t)rem * W * elem;
    emit(dev_to_dev && !same_device ? RT_COPY_PEER : RT_COPY_LINEAR, d0 + (size_t)full * N * band_bytes, 0,
         (size_t)full * band_bytes, 0, bytes, 1);
  }
  return cnt;
}

static int deliver_bands(rt_ctx* p, int k, const void* stripe, void* dst, size_t elem, hipMemcpyKind kind, hipStream_t stream) {
  rt_ctx* c = p->kids[k];
  const int N = (int)p->kids.size(), dbr = p->cfg.device_band_rows, W = p->cfg.width;
  const bool d2d = kind == hipMemcpyDeviceToDevice;
  const int full = c->owned_rows / dbr;
  std::vector<rt_band_copy> plan((size_t)full + 2);
  int cnt = band_copy_plan(N, k, dbr, W, c->owned_rows, elem, d2d, c->peer_ok, c->device == p->device, plan.data(), (int)plan.size());
  for (int i = 0; i < cnt; ++i) {
    const rt_band_copy& q = plan[(size_t)i];
    char* const d = (char*)dst + q.dst_offset;
    const char* const sp = (const char*)stripe + q.src_offset;
    if (q.op == RT_COPY_2D) {
      const hipError_t e = hipMemcpy2DAsync(d, q.dst_pitch, sp, q.src_pitch, q.width_bytes, q.rows, kind, stream);
      if (e != hipSuccess && d2d && c->device != p->device) {
        // the direct 2-D copy was refused after all: from now on this device copies band by band through the runtime
        (void)hipGetLastError();
        c->peer_ok = false;
        set_error("warning: device %d cannot copy 2-D into device %d (%s): its bands go band by band through hipMemcpyPeerAsync",
                  c->device, p->device, hipGetErrorString(e));
        cnt = band_copy_plan(N, k, dbr, W, c->owned_rows, elem, d2d, false, false, plan.data(), (int)plan.size());
        i = -1;
        continue;
      }
      if (e != hipSuccess) { set_error("hipMemcpy2DAsync failed: %s", hipGetErrorString(e)); return RT_E_DEVICE; }
    } else if (q.op == RT_COPY_PEER) {
      HIP_TRY(hipMemcpyPeerAsync(d, p->device, sp, c->device, q.width_bytes, stream));
    } else {
      HIP_TRY(hipMemcpyAsync(d, sp, q.width_bytes, kind, stream));
    }
  }
  return RT_OK;
}

static int parent_render(rt_ctx* p, const float rot[12], const float cam[3], const float light[3], float focal,
                         uint32_t* host_argb, float* host_rgb, uint32_t* d_argb, float4* d_rgb, hipStream_t caller) {
  const bool to_host = host_argb != nullptr;
  const size_t W = (size_t)p->cfg.width;
  const size_t nk = p->kids.size();
  if (!to_host) {                                     // the caller's earlier work on the destination comes first
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipEventRecord(p->ev0, caller));
    HIP_TRY(hipEventRecord(p->ev_go, caller));
  }
  const bool want_rgb = to_host ? host_rgb != nullptr : d_rgb != nullptr;
  std::vector<char> launched(nk, 0), direct(nk, 0);
  // On an error the devices already launched may still be writing into the caller's buffers: wait for them before returning
  auto fail = [&](int rc) {
    KeepError keep;
    for (size_t k = 0; k < nk; ++k)
      if (launched[k]) { hipSetDevice(p->kids[k]->device); hipStreamSynchronize(p->kids[k]->stream); }
    (void)hipGetLastError();
    return rc;
  };
  // pass 1: every device's frame is launched before any band is delivered.  (Delivering inside this loop made the host
  // thread wait for device k's kernel and copy — a device-to-pageable-host copy blocks — before it launched device k+1:
  // the devices then ran one after another.)
  for (size_t k = 0; k < nk; ++k) {
    rt_ctx* c = p->kids[k];
    if (c->owned_rows == 0) continue;
    if (hipSetDevice(c->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", c->device); return fail(RT_E_DEVICE); }
    if (want_rgb && !c->d_rgb && c->d_rgb.alloc((size_t)c->owned_rows * W) != hipSuccess) {
      set_error("hipMalloc failed (float tap, device %d)", c->device); return fail(RT_E_NOMEM);
    }
    if (!to_host && hipStreamWaitEvent(c->stream, p->ev_go, 0) != hipSuccess) { set_error("hipStreamWaitEvent failed"); return fail(RT_E_DEVICE); }
    // a device that holds the destination writes its rows there itself; the others render into their stripe.  A registered
    // host framebuffer (rt_register_output) is held by every device: each writes its bands into it over its own PCIe link.
    const bool mapped = to_host && !host_rgb && c->reg_host && (char*)host_argb >= c->reg_host &&
                        (char*)host_argb + (size_t)p->cfg.height * W * 4 <= c->reg_host + c->reg_bytes &&
                        !(p->cfg.flags & RT_FLAG_STAGED_GATHER);
    direct[k] = mapped || (!to_host && c->device == p->device && !(p->cfg.flags & RT_FLAG_STAGED_GATHER));
    uint32_t* const dst = mapped ? reinterpret_cast<uint32_t*>(c->reg_dev + ((char*)host_argb - c->reg_host)) : d_argb;
    const int rc = direct[k] ? launch_frame(c, rot, cam, light, focal, dst, mapped ? nullptr : d_rgb, c->stream, true)
                             : launch_frame(c, rot, cam, light, focal, c->d_argb, want_rgb ? c->d_rgb : nullptr, c->stream);
    if (rc != RT_OK) return fail(rc);
    launched[k] = 1;
  }
  // pass 2: the copy engines deliver the bands, every device on its own stream behind its own kernel
  for (size_t k = 0; k < nk; ++k) {
    rt_ctx* c = p->kids[k];
    if (!launched[k]) continue;
    if (hipSetDevice(c->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", c->device); return fail(RT_E_DEVICE); }
    if (!direct[k]) {
      const hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
      int rc = deliver_bands(p, (int)k, c->d_argb, to_host ? (void*)host_argb : (void*)d_argb, 4, kind, c->stream);
      if (rc == RT_OK && want_rgb)
        rc = deliver_bands(p, (int)k, c->d_rgb, to_host ? (void*)host_rgb : (void*)d_rgb, sizeof(float4), kind, c->stream);
      if (rc != RT_OK) return fail(rc);
    }
    if (!to_host && hipEventRecord(c->ev_done, c->stream) != hipSuccess) { set_error("hipEventRecord failed"); return fail(RT_E_DEVICE); }
  }
  if (to_host) {
    for (rt_ctx* c : p->kids) if (c->owned_rows) { HIP_TRY(hipSetDevice(c->device)); HIP_TRY(hipStreamSynchronize(c->stream)); }
    p->timed = false;             // rt_last_kernel_ms: this frame's time is the children's, not an older device-path interval
  } else {
    HIP_TRY(hipSetDevice(p->device));
    for (rt_ctx* c : p->kids) if (c->owned_rows) HIP_TRY(hipStreamWaitEvent(caller, c->ev_done, 0));
    HIP_TRY(hipEventRecord(p->ev1, caller));
    p->timed = true;
  }
  return RT_OK;
}

extern "C" {

int rt_render_device(rt_ctx* c, const float rot[12], const float cam[3], const float light[3], float focal,
                     void* d_out_argb, void* d_out_rgb_f32, void* hip_stream) {
  if (!c || !d_out_argb) { set_error("NULL argument"); return RT_E_INVALID; }
  DeviceGuard guard;
  if (!c->kids.empty()) {
    if (!rot || !cam || !light) { set_error("NULL argument"); return RT_E_INVALID; }
    return parent_render(c, rot, cam, light, focal, nullptr, nullptr, (uint32_t*)d_out_argb, (float4*)d_out_rgb_f32, (hipStream_t)hip_stream);
  }
  return launch_frame(c, rot, cam, light, focal, (uint32_t*)d_out_argb, (float4*)d_out_rgb_f32, (hipStream_t)hip_stream);
}

int rt_render(rt_ctx* c, const float rot[12], const float cam[3], const float light[3], float focal,
              uint32_t* out_argb, float* out_rgb_f32) {
  if (!c || !out_argb) { set_error("NULL argument"); return RT_E_INVALID; }
  DeviceGuard guard;
  if (!c->kids.empty()) {
    if (!rot || !cam || !light) { set_error("NULL argument"); return RT_E_INVALID; }
    return parent_render(c, rot, cam, light, focal, out_argb, out_rgb_f32, nullptr, nullptr, nullptr);
  }
  const size_t px = (size_t)c->owned_rows * c->cfg.width;
  if (out_rgb_f32 && !c->d_rgb) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->d_rgb.alloc(px));
  }
  if (c->reg_host && !out_rgb_f32 && px != 0 && (char*)out_argb >= c->reg_host &&
      (char*)out_argb + px * 4 <= c->reg_host + c->reg_bytes) {
    // the caller's framebuffer is mapped: the kernel's stores ARE the read-back (rt_register_output)
    uint32_t* const d_out = reinterpret_cast<uint32_t*>(c->reg_dev + ((char*)out_argb - c->reg_host));
    const int rc0 = launch_frame(c, rot, cam, light, focal, d_out, nullptr, c->stream);
    if (rc0 != RT_OK) return rc0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RT_OK;
  }
  int rc = launch_frame(c, rot, cam, light, focal, c->d_argb, out_rgb_f32 ? c->d_rgb : nullptr, c->stream);
  if (rc != RT_OK) return rc;
  if (px == 0) return RT_OK;
  // blocking readback, as clEnqueueReadBuffer(CL_TRUE) at skeleton.cpp:179
  HIP_TRY(hipMemcpyAsync(out_argb, c->d_argb, px * 4, hipMemcpyDeviceToHost, c->stream));
  if (out_rgb_f32) HIP_TRY(hipMemcpyAsync(out_rgb_f32, c->d_rgb, px * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RT_OK;
}

int rt_unregister_output(rt_ctx* c) {
  if (!c) { set_error("NULL argument"); return RT_E_INVALID; }
  if (!c->reg_host || !c->reg_owner) return RT_OK;
  DeviceGuard guard;
  for (rt_ctx* k : c->kids) {                        // no frame of any device may still be writing
    HIP_TRY(hipSetDevice(k->device));
    HIP_TRY(hipStreamSynchronize(k->stream));
    k->reg_host = k->reg_dev = nullptr; k->reg_bytes = 0;
  }
  HIP_TRY(hipSetDevice(c->device));
  if (c->timed) HIP_TRY(hipEventSynchronize(c->ev1));
  HIP_TRY(hipHostUnregister(c->reg_host));
  c->reg_host = c->reg_dev = nullptr; c->reg_bytes = 0; c->reg_owner = false;
  return RT_OK;
}

int rt_register_output(rt_ctx* c, void* host, size_t bytes) {
  if (!c || !host || bytes == 0) { set_error("NULL argument"); return RT_E_INVALID; }
  const int rc = rt_unregister_output(c);
  if (rc != RT_OK) return rc;
  DeviceGuard guard;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipHostRegister(host, bytes, hipHostRegisterMapped | hipHostRegisterPortable));
  auto alias = [&](rt_ctx* x) -> bool {              // the range as device x->device addresses it
    void* dev = nullptr;
    if (hipSetDevice(x->device) != hipSuccess || hipHostGetDevicePointer(&dev, host, 0) != hipSuccess || !dev) return false;
    x->reg_host = static_cast<char*>(host); x->reg_dev = static_cast<char*>(dev); x->reg_bytes = bytes;
    return true;
  };
  bool ok = alias(c);
  for (rt_ctx* k : c->kids) ok = ok && alias(k);
  if (!ok) {
    for (rt_ctx* k : c->kids) { k->reg_host = k->reg_dev = nullptr; k->reg_bytes = 0; }
    c->reg_host = c->reg_dev = nullptr; c->reg_bytes = 0;
    hipHostUnregister(host);
    set_error("hipHostGetDevicePointer failed: %s", hipGetErrorString(hipGetLastError()));
    return RT_E_DEVICE;
  }
  c->reg_owner = true;
  return RT_OK;
}

// Both counting calls, on the context's own stream: rt_count_work's pass (the thread-per-pixel kernel, the reference's
// semantics) or, `executed`, rt_count_executed's (the counting build of what renders the frame).  Behind what rewrites the
// scene or shares the frames' buffers — the executed pass behind the previous frame too, whose queues and records it uses
//  —, the counters cleared, the instrumented launch, the blocking read-back.  Several devices: the children's sum
static int count_frame(rt_ctx* c, const float rot[12], const float cam[3], const float light[3], float focal, bool executed,
                       uint64_t out[8]) {
  static_assert(sizeof(rt_work) == 8 * sizeof(uint64_t), "rt_work is eight counters");
  if (!c || !out || !rot || !cam || !light) { set_error("NULL argument"); return RT_E_INVALID; }
  memset(out, 0, sizeof(rt_work));
  DeviceGuard guard;
  for (rt_ctx* k : c->kids) {
    uint64_t w[8];
    const int rc = count_frame(k, rot, cam, light, focal, executed, w);
    if (rc != RT_OK) return rc;
    for (int q = 0; q < 8; ++q) out[q] += w[q];
  }
  if (!c->kids.empty() || c->owned_rows == 0) return RT_OK;
  FrameParams P;
  fill_params(c, rot, cam, light, focal, &P);
  const Family family = executed ? frame_family(c, P) : Family::generic;
  if (executed && (family == Family::generic || (family == Family::wave && !wave_can_count(P, frame_cull(c))))) {
    // (two texts, as ever: the chunked build's frames are told of it, every other frame — one of more than 64 shadow samples
    // on the wave kernel too — of rt_count_work)
    set_error("%s", family == Family::wave && P.aa_x * P.aa_y > 64
                  ? "rt_count_executed: more than 64 AA samples per pixel run on the wave kernel's chunked build, which has no counting build"
                  : "rt_count_executed: this configuration runs on the generic kernel, whose executed work is rt_count_work");
    return RT_E_UNSUPPORTED;
  }
  P.counters = c->d_counters;
  HIP_TRY(hipSetDevice(c->device));
  if (executed && c->timed) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev1, 0));
  HIP_TRY(wait_aov(c, c->stream));
  HIP_TRY(wait_scene(c, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_counters, 0, sizeof(rt_work), c->stream));
  if (family == Family::generic) launch_generic(P, true, c->stream);
  else if (family == Family::wave) launch_wave(P, frame_cull(c), true, c->tune.phase_profile, c->stream);   // (phase_profile: s_memtime per phase)
  else { use_tiled_scene(c, &P); launch_stage_records(P, c->stream); launch_mesh(P, true, c->tune.phase_profile, c->stream, nullptr, nullptr, nullptr); }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, c->d_counters, sizeof(rt_work), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RT_OK;
}

int rt_count_work(rt_ctx* c, const float rot[12], const float cam[3], const float light[3], float focal, rt_work* out) {
  return count_frame(c, rot, cam, light, focal, false, reinterpret_cast<uint64_t*>(out));
}

int rt_count_executed(rt_ctx* c, const float rot[12], const float cam[3], const float light[3], float focal, uint64_t out[8]) {
  return count_frame(c, rot, cam, light, focal, true, out);
}

int rt_debug_wave_timeline(rt_ctx* c, uint64_t out[8]) {
  if (!c || !out) { set_error("NULL argument"); return RT_E_INVALID; }
  c = lead_ctx(c);
  if (!c->tune.timeline || !c->timeline_valid) {
    set_error("rt_debug_wave_timeline: needs UOB_RT_TIMELINE=1 at rt_init and a frame rendered by the wave kernel");
    return RT_E_UNSUPPORTED;
  }
  DeviceGuard guard;
  HIP_TRY(hipSetDevice(c->device));
  if (c->timed) HIP_TRY(hipEventSynchronize(c->ev1));
  std::vector<uint64_t> rec(c->timeline_waves * 3);
  HIP_TRY(hipMemcpy(rec.data(), c->d_timeline, rec.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  for (int q = 0; q < 8; ++q) out[q] = 0;
  out[1] = ~0ull;
  for (size_t w = 0; w < c->timeline_waves; ++w) {
    const uint64_t t0 = rec[3 * w], t1 = rec[3 * w + 1], jobs = rec[3 * w + 2] & 0xffffffffull;
    if (t1 == 0) continue;                  // a slot no wave of the grid wrote
    out[7] = rec[3 * w + 2] >> 32;
    out[0] += 1; out[3] += t0; out[4] += t1; out[5] += jobs;
    if (t0 < out[1]) out[1] = t0;
    if (t1 > out[2]) out[2] = t1;
    if (jobs > out[6]) out[6] = jobs;
  }
  return RT_OK;
}

// What both views of the last frame's seed table share: the argument check, dims, the table and per tile the rows of it the
// context renders (each of them is one job per column, and every job reads its tile's record), `view` over every record with
// its rows, the copy into the caller's array.  An empty table when the last frame took no seed
static int seed_table_view(rt_ctx* c, void* records, int64_t cap, int32_t dims[3], uint64_t* counters, int ncounters,
                           void (*view)(SeedRec& r, uint64_t rows, uint64_t* counters)) {
  if (!c || !dims || !counters || cap < 0 || (cap > 0 && !records)) { set_error("NULL argument"); return RT_E_INVALID; }
  c = lead_ctx(c);
  dims[0] = c->seed_tile_rows; dims[1] = c->seed_nseg; dims[2] = c->seed_rows;
  for (int q = 0; q < ncounters; ++q) counters[q] = 0;
  if (c->seed_tile_rows == 0) { dims[1] = 0; return RT_OK; }
  DeviceGuard guard;
  HIP_TRY(hipSetDevice(c->device));
  if (c->timed) HIP_TRY(hipEventSynchronize(c->ev1));
  std::vector<SeedRec> rec((size_t)c->seed_tile_rows * (size_t)c->seed_nseg);
  HIP_TRY(hipMemcpy(rec.data(), c->d_seed, rec.size() * sizeof(SeedRec), hipMemcpyDeviceToHost));
  const rt_config& g = c->cfg;
  for (int tr = 0; tr < c->seed_tile_rows; ++tr) {
    uint64_t rows = 0;
    for (int y = tr * c->seed_rows; y < (tr + 1) * c->seed_rows && y < g.height; ++y)
      rows += ((y / g.band_rows) % g.band_count) == g.band_index;
    for (int col = 0; col < c->seed_nseg; ++col) view(rec[(size_t)tr * (size_t)c->seed_nseg + (size_t)col], rows, counters);
  }
  if (records) memcpy(records, rec.data(), (size_t)((int64_t)rec.size() < cap ? (int64_t)rec.size() : cap) * sizeof(SeedRec));
  return RT_OK;
}

// The strict view: the strict bits alone, and nothing of a part whose strict bit is not set
int rt_debug_wave_seeds(rt_ctx* c, void* records, int64_t cap, int32_t dims[3], uint64_t counters[4]) {
  return seed_table_view(c, records, cap, dims, counters, 4, [](SeedRec& r, uint64_t n, uint64_t* counters) {
    r.flags &= kSeedPrimary | kSeedShadow;
    if (!(r.flags & kSeedPrimary)) r.Kp = 0ull;
    if (!(r.flags & kSeedShadow)) { r.D0[0] = r.D0[1] = r.D0[2] = 0.0f; r.ed = 0.0f; r.K = 0ull; r.Kh = 0ull; r.h = -1; }
    if (r.flags & kSeedPrimary) { counters[0] += 1; counters[2] += n; }
    if (r.flags & kSeedShadow) { counters[1] += 1; counters[3] += n; }
  });
}

// The records as the draw kernel reads them
int rt_debug_wave_seeds_wide(rt_ctx* c, void* records, int64_t cap, int32_t dims[3], uint64_t counters[10]) {
  return seed_table_view(c, records, cap, dims, counters, 10, [](SeedRec& r, uint64_t n, uint64_t* counters) {
    const bool shadow = (r.flags & kSeedShadowWide) != 0u;
    const bool is[5] = {(r.flags & kSeedPrimaryWide) != 0u, shadow, shadow && r.Kh != 0ull, shadow && (r.flags & kSeedShadowSph) != 0u,
                        shadow && (r.flags & kSeedShadowBlocked) != 0u};
    for (int q = 0; q < 5; ++q)
      if (is[q]) { counters[2 * q] += 1; counters[2 * q + 1] += n; }
  });
}

int rt_debug_trace_rays(rt_ctx* c, int32_t what, const float* rays6, const float* radius_sq, int64_t nray,
                        int32_t* out_tri, float* out10) {
  if (!c || !rays6 || !out_tri || nray < 0) { set_error("NULL argument"); return RT_E_INVALID; }
  if (what != RT_TRACE_IN_SHADOW && what != RT_TRACE_CLOSEST_HIT) { set_error("rt_debug_trace_rays: unknown mode %d", what); return RT_E_INVALID; }
  if (what == RT_TRACE_IN_SHADOW && !radius_sq) { set_error("rt_debug_trace_rays: radius_sq missing"); return RT_E_INVALID; }
  if (what == RT_TRACE_CLOSEST_HIT && !out10) { set_error("rt_debug_trace_rays: out10 missing"); return RT_E_INVALID; }
  c = lead_ctx(c);
  if (nray == 0) return RT_OK;
  DeviceGuard guard;
  HIP_TRY(hipSetDevice(c->device));
  const float zero3[3] = {0.f, 0.f, 0.f};
  FrameParams P;
  scene_params(c, zero3, false, &P);
  DevMem<float> d_rays, d_r2, d_out;           // (after the guard: freed while the context's device is current)
  DevMem<int> d_tri;
  const size_t n = (size_t)nray;
  if (d_rays.alloc(n * 6) != hipSuccess || d_tri.alloc(n) != hipSuccess || (radius_sq && d_r2.alloc(n) != hipSuccess) ||
      (out10 && d_out.alloc(n * 10) != hipSuccess))
    return alloc_failed();
  if (c->timed) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev1, 0));
  HIP_TRY(wait_aov(c, c->stream));
  HIP_TRY(wait_scene(c, c->stream));
  HIP_TRY(hipMemcpyAsync(d_rays, rays6, n * 24, hipMemcpyHostToDevice, c->stream));
  if (radius_sq) HIP_TRY(hipMemcpyAsync(d_r2, radius_sq, n * 4, hipMemcpyHostToDevice, c->stream));
  if (d_out) HIP_TRY(hipMemsetAsync(d_out, 0, n * 40, c->stream));
  if (generic_needs_records(c->n)) launch_stage_records(P, c->stream);
  launch_trace_rays(P, what, d_rays, d_r2, (long)nray, d_tri, d_out, c->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_tri, d_tri, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (out10 && what == RT_TRACE_CLOSEST_HIT) HIP_TRY(hipMemcpyAsync(out10, d_out, n * 40, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));    // (on an earlier failure the owners' hipFree waits for what was enqueued)
  return RT_OK;
}

int rt_debug_band_copy_plan(int32_t num_devices, int32_t k, int32_t device_band_rows, int32_t width, int32_t height,
                            int32_t elem_bytes, int32_t dev_to_dev, int32_t peer_ok, int32_t same_device,
                            rt_band_copy* out, int32_t cap) {
  if (num_devices < 1 || num_devices > RT_MAX_DEVICES || k < 0 || k >= num_devices || device_band_rows < 0 || width < 1 ||
      height < 1 || elem_bytes < 1 || cap < 0 || (!out && cap > 0)) {
    set_error("rt_debug_band_copy_plan: invalid argument"); return RT_E_INVALID;
  }
  const int dbr = device_band_rows > 0 ? device_band_rows : 32;
  rt_config kc;
  memset(&kc, 0, sizeof kc);
  kc.height = height; kc.band_rows = dbr; kc.band_index = k; kc.band_count = num_devices;
  return band_copy_plan(num_devices, k, dbr, width, rt_config_owned_rows(&kc), (size_t)elem_bytes, dev_to_dev != 0, peer_ok != 0,
                        same_device != 0, out, cap);
}

int rt_debug_block_costs(rt_ctx* c, uint32_t* out, int32_t cap) {
  if (!c || (!out && cap > 0) || cap < 0) { set_error("NULL argument"); return RT_E_INVALID; }
  c = lead_ctx(c);
  if (!c->d_mesh_cost || !c->mesh_order_valid) { set_error("rt_debug_block_costs: this context records no block costs"); return RT_E_UNSUPPORTED; }
  DeviceGuard guard;
  HIP_TRY(hipSetDevice(c->device));
  const int jobs = ((c->cfg.width + 15) / 16) * ((c->owned_rows + 15) / 16);
  if (c->timed) HIP_TRY(hipEventSynchronize(c->ev1));
  // job id -> block: rows are numbered from the middle outwards (rt_kernel_mesh.hip), undo that here
  std::vector<uint32_t> raw((size_t)jobs);
  HIP_TRY(hipMemcpy(raw.data(), c->d_mesh_cost, (size_t)jobs * 4, hipMemcpyDeviceToHost));
  const int wx = (c->cfg.width + 15) / 16, wy = (c->owned_rows + 15) / 16, mid = (wy + 1) >> 1;
  for (int j = 0; j < jobs; ++j) {
    const int jy = j / wx, jx = j - jy * wx;
    const int row = (jy & 1) ? mid + (jy >> 1) : mid - 1 - (jy >> 1);
    const int at = row * wx + jx;
    if (at >= 0 && at < cap) out[at] = raw[(size_t)j];
  }
  return jobs;
}

int rt_debug_world_masks(rt_ctx* c, uint64_t* out, int64_t cap, int32_t* grid, int32_t* words) {
  if (!c || (!out && cap > 0) || cap < 0 || !grid || !words) { set_error("NULL argument"); return RT_E_INVALID; }
  c = lead_ctx(c);
  if (!c->d_world_masks || c->nwords <= 0) { set_error("rt_debug_world_masks: this context builds no tile masks"); return RT_E_UNSUPPORTED; }
  DeviceGuard guard;
  HIP_TRY(hipSetDevice(c->device));
  if (c->timed) HIP_TRY(hipEventSynchronize(c->ev1));
  const size_t total = (size_t)kWorldGrid * kWorldGrid * kWorldGrid * (size_t)c->nwords;
  *grid = kWorldGrid; *words = c->nwords;
  const size_t take = total < (size_t)cap ? total : (size_t)cap;
  if (take > 0) HIP_TRY(hipMemcpy(out, c->d_world_masks, take * 8, hipMemcpyDeviceToHost));
  return (int)total;
}

int rt_last_kernel_ms(rt_ctx* c, float* out_ms) {
  if (!c || !out_ms) { set_error("NULL argument"); return RT_E_INVALID; }
  DeviceGuard guard;
  if (!c->kids.empty() && !c->timed) {      // after rt_render into host memory: the slowest device's kernel
    float mx = -1.0f;
    for (rt_ctx* k : c->kids) {
      float ms = 0.0f;
      if (k->timed && rt_last_kernel_ms(k, &ms) == RT_OK && ms > mx) mx = ms;
    }
    if (mx < 0.0f) { set_error("no frame has been rendered on this context"); return RT_E_INVALID; }
    *out_ms = mx;
    return RT_OK;
  }
  if (!c->timed) { set_error("no frame has been rendered on this context"); return RT_E_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->ev1));
  HIP_TRY(hipEventElapsedTime(out_ms, c->ev0, c->ev1));
  return RT_OK;
}

int rt_debug_live_device_objects(int64_t out[4]) {
  if (!out) { set_error("rt_debug_live_device_objects: NULL argument"); return RT_E_INVALID; }
  for (int k = 0; k < 4; ++k) out[k] = g_live[k].load(std::memory_order_relaxed);
  return RT_OK;
}

void rt_destroy(rt_ctx* c) {
  if (!c) return;
  DeviceGuard guard;
  delete c;
}

}  // extern "C"

// What only the context can do before its members release themselves: the children first, then its own device current and
// nothing of it still running
rt_ctx::~rt_ctx() {
  for (rt_ctx* k : kids) delete k;
  hipSetDevice(device);
  if (stream) hipStreamSynchronize(stream);
  if (aux_stream) hipStreamSynchronize(aux_stream);
  for (SideCall* k : {&query, &shade, &rad, &aov, &filter, &accum, &motion})     // no call of any family may still be running
    if (k->ev) hipEventSynchronize(k->ev);
  if (reg_host && reg_owner) hipHostUnregister(reg_host);
}
