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
// Here: contexts, frames, delivery across devices, scene updates, output registration and diagnostics.  The calls beside
// the frame (ray queries, shade and radiance calls, AOV passes) are rt_calls.hip; the context itself is rt_host.h.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

}  // namespace uobrt

using namespace uobrt;

constexpr int kWorldGrid = 32;       // world cells per axis of the mesh kernel's shadow-ray tile masks

// rt_init's and rt_update_spheres' bounds of a sphere table (the count is checked by the caller)
static int validate_spheres(const rt_sphere* sph, int num) {
  for (int i = 0; i < num; ++i) {
    const rt_sphere& s = sph[i];
    for (int k = 0; k < 3; ++k)
      if (!(fabsf(s.center[k]) <= kMaxCoordinate)) { set_error("sphere %d: |centre| must be finite and <= 2^16", i); return RT_E_INVALID; }
    if (!(fabsf(s.radius_sq) <= kMaxCoordinate * kMaxCoordinate)) { set_error("sphere %d: radius_sq must be finite and <= 2^32", i); return RT_E_INVALID; }
  }
  return RT_OK;
}

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
  return t;
}

// Coordinate bound: the range over which the exact culls are verified and which keeps every
// determinant of the intersection tests below 2^126, where the v_rcp_f32 + Newton reciprocal equals IEEE
// division bit for bit (rt_math.h rcp_exact).
static int validate_vertices(const float* vertices4, int n) {
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

// The context's sphere table (cfg.spheres) into device memory; blocking
static int upload_spheres(rt_ctx* c) {
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

static int scene_first(rt_ctx* c, const float* v4, const float* n4, const float* c4, int n);   // below, with the scene updates

static int upload_tiled_scene(rt_ctx* c, const float* v4, const float* n4, const float* c4) {
  const std::vector<int> orig = tiled_order(v4, c->n, c->tune.tile_morton);
  return upload_tiled(c, v4, n4, c4, orig, tile_data_host(v4, orig.data(), c->n));
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

static int init_parent(const rt_config* cfg, const float* vertices4, const float* normals4, const float* colors4,
                       int32_t n, rt_ctx** out_ctx) {
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev < 1) { set_error("no HIP device present"); return RT_E_DEVICE; }
  for (int d = 0; d < cfg->num_devices; ++d)
    if (cfg->devices[d] < 0 || cfg->devices[d] >= ndev) {
      set_error("devices[%d] = %d, but %d HIP device(s) are present", d, cfg->devices[d], ndev); return RT_E_INVALID;
    }
  rt_ctx* p = new (std::nothrow) rt_ctx();
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
    if (rc != RT_OK) { rt_destroy(p); return rc; }
    p->kids.push_back(k);
    if (hipSetDevice(k->device) != hipSuccess || hipEventCreateWithFlags(&k->ev_done, hipEventDisableTiming) != hipSuccess) {
      set_error("event creation failed on device %d", k->device); rt_destroy(p); return RT_E_DEVICE;
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
  if (hipSetDevice(p->device) != hipSuccess || hipEventCreateWithFlags(&p->ev_go, hipEventDisableTiming) != hipSuccess ||
      hipStreamCreate(&p->stream) != hipSuccess || hipEventCreate(&p->ev0) != hipSuccess || hipEventCreate(&p->ev1) != hipSuccess) {
    set_error("stream/event creation failed on device %d", p->device); rt_destroy(p); return RT_E_DEVICE;
  }
  // RT_OK with a "warning: ..." line in rt_last_error(): the context works, through the slower copies
  if (!downgrade.empty()) set_error("%s: their bands are copied band by band (hipMemcpyPeerAsync)", downgrade.c_str());
  *out_ctx = p;
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
  if (n > 4000000) { set_error("triangle list of %d exceeds the supported maximum of 4000000", n); return RT_E_UNSUPPORTED; }
  DeviceGuard guard;
  if (cfg->num_devices > 1) return init_parent(cfg, vertices4, normals4, colors4, n, out_ctx);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev < 1) { set_error("no HIP device present"); return RT_E_DEVICE; }
  rt_ctx* c = new (std::nothrow) rt_ctx();
  if (!c) { set_error("out of host memory"); return RT_E_NOMEM; }
  c->cfg = *cfg;
  c->tune = read_tuning(*cfg);
  if (cfg->num_devices == 1) c->device = cfg->devices[0];
  else if (cfg->device >= 0) c->device = cfg->device;
  else hipGetDevice(&c->device);
  auto fail = [&](int code) { rt_destroy(c); return code; };
  if (hipSetDevice(c->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", c->device); return fail(RT_E_DEVICE); }
  c->owned_rows = rt_config_owned_rows(cfg);
  if (hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || c->cus < 1) c->cus = 256;
  const size_t px = (size_t)(c->owned_rows > 0 ? c->owned_rows : 1) * cfg->width;
  if (hipMalloc(&c->d_argb, px * 4) != hipSuccess || hipMalloc(&c->d_counters, sizeof(rt_work)) != hipSuccess ||
      hipMalloc(&c->d_jobctr, (2 * kJobHeads + 2) * kJobHeadStride * sizeof(unsigned int)) != hipSuccess ||
      hipMalloc(&c->d_spheres, RT_MAX_SPHERES * sizeof(DevSphere)) != hipSuccess) {
    set_error("hipMalloc failed: %s", hipGetErrorString(hipGetLastError())); return fail(RT_E_NOMEM);
  }
  {   // wave kernel: lists of last frame's expensive jobs (sized for the smallest job, one 64-ray task)
    const int aa = cfg->aa_x * cfg->aa_y;
    const int pt = (aa >= 1 && aa <= 64) ? 64 / aa : 16;        // smallest job: one task; more than 64 AA samples: 16 pixels
    const size_t jobs_max = (size_t)((cfg->width + pt - 1) / pt) * (size_t)(c->owned_rows > 0 ? c->owned_rows : 1);
    c->heavy_cap = (int)(jobs_max / 3 > 64 ? jobs_max / 3 : 64);
    c->heavy_jobs_max = jobs_max;
  }
  if (hipStreamCreate(&c->stream) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
    set_error("stream/event creation failed"); return fail(RT_E_DEVICE);
  }
  rc = upload_spheres(c);
  if (rc != RT_OK) return fail(rc);
  // the scene: buffers by n, upload, tiles, n_shadow, scene box, kernel family — the routine rt_replace_scene calls too
  rc = scene_first(c, vertices4, normals4, colors4, n);
  if (rc != RT_OK) return fail(rc);
  *out_ctx = c;
  return RT_OK;
}

}  // extern "C"

void uobrt::fill_params(const rt_ctx* c, const float rot[12], const float cam[3], const float light[3], float focal,
                        FrameParams* P) {
  memset(P, 0, sizeof *P);
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
  {   // wave kernel: a job is a run of job_tasks 64-ray tasks (job_tasks * 64/aa pixels) of one row
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
  if (c->d_screen_masks) {
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
}

// The mesh kernel works on the reordered copy of the scene (upload_tiled_scene)
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
  const bool wave_paths = !(c->cfg.flags & RT_FLAG_GENERIC_KERNEL);
  if (wave_paths && wave_kernel_supports(P) && (P.aa_x * P.aa_y <= 64 || !(c->cfg.flags & RT_FLAG_NO_CULL))) {
    // last frame's expensive jobs first — where jobs are long enough (4+ tasks) for the extra look-up per
    // hand-out not to matter (measured: 1024^2 frames with 16-pixel jobs lose 12-18 % to it, larger ones gain 2-8 %)
    if (c->d_heavy_flags && P.job_tasks >= 4) {
      const int prev = c->heavy_phase, cur = prev ^ 1;
      unsigned int* const st[2] = {c->d_jobctr, c->d_jobctr + (2 * kJobHeads + 1) * kJobHeadStride};
      P.heavy_prev = c->d_heavy[prev]; P.heavy_prev_state = st[prev];
      P.heavy_new = c->d_heavy[cur]; P.heavy_new_state = st[cur];
      P.heavy_flags = c->d_heavy_flags + (size_t)prev * c->heavy_jobs_max; P.heavy_flags_new = c->d_heavy_flags + (size_t)cur * c->heavy_jobs_max;
      P.heavy_gen = ++c->heavy_gen;
      P.heavy_factor4 = c->tune.heavy_factor4;                      // expensive = more than twice the average job
      P.heavy_cap = P.njobs / 3 < c->heavy_cap ? P.njobs / 3 : c->heavy_cap;
      P.heavy_dilate = c->tune.heavy_dilate ? 1 : 0;
      c->heavy_phase = cur;
    }
    c->timeline_valid = false;
    if (c->tune.timeline) {                 // diagnostic: the shipped kernel, with its per-wave start / end stamps
      const size_t waves = (size_t)P.wave_blocks * 4;
      if (!c->d_timeline) {
        if (hipMalloc(&c->d_timeline, waves * 3 * sizeof(uint64_t)) != hipSuccess) { set_error("hipMalloc failed (timeline)"); return RT_E_NOMEM; }
        c->timeline_waves = waves;
      }
      if (c->timeline_waves >= waves) {
        HIP_TRY(hipMemsetAsync(c->d_timeline, 0, c->timeline_waves * 3 * sizeof(uint64_t), stream));
        P.counters = reinterpret_cast<unsigned long long*>(c->d_timeline);
        c->timeline_valid = true;
      }
    }
    launch_wave(P, !(c->cfg.flags & RT_FLAG_NO_CULL), false, stream);
  } else if (wave_paths && !(c->cfg.flags & RT_FLAG_NO_CULL) && mesh_kernel_supports(P)) {
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

// ---- scene updates (rt_update_scene / rt_update_scene_device) ----------------------------------------------
// The tiling of rt_init is kept: tile membership is a free choice (the closest hit resolves ties by the original index,
// d_orig), so only the tiles' data are recomputed for the new vertices (rt_scene_update.hip rt_scene_refit), unless the
// caller asks for the tiles to be sorted again (RT_UPDATE_REORDER: the rt_init path on the host).

// An update enqueued on `s` first waits for everything that may still read the buffers it overwrites: the context's
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

// ---- the scene of a context: rt_init's first one and every replacement (rt_replace_scene*) ---------------------------
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
  float4 *verts = nullptr, *normals = nullptr, *colors = nullptr;
  SceneStore t;
};

static void free_growth(SceneGrowth* g) {
  hipFree(g->verts); hipFree(g->normals); hipFree(g->colors); hipFree(g->t.records);
  hipFree(g->t.verts_m); hipFree(g->t.normals_m); hipFree(g->t.colors_m); hipFree(g->t.orig); hipFree(g->t.tile_box);
  hipFree(g->t.screen_masks); hipFree(g->t.world_masks);
  *g = SceneGrowth();
}

// Everything a scene of n triangles needs that the context does not hold yet.  Nothing the context renders from is touched:
// what outgrows the capacity goes into *g; what the context meets for the first time (the buffers of a kernel family it has
// not run yet) goes into its store, which no frame reads before scene_select.  device_tiles: the device tile build will run.
static int scene_reserve(rt_ctx* c, int n, bool device_tiles, SceneGrowth* g) {
  if (hipSetDevice(c->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", c->device); return RT_E_DEVICE; }
  const SceneNeeds q = scene_needs(c, n);
  const rt_config& cfg = c->cfg;
  SceneStore& o = c->own;
  bool ok = true;
  auto get = [&](auto** p, size_t bytes) { if (ok && hipMalloc(p, bytes ? bytes : 1) != hipSuccess) ok = false; };
  auto tiled_set = [&](SceneStore* t, int cap) {
    const size_t nb = (size_t)cap * sizeof(float4);
    get(&t->verts_m, 3 * nb); get(&t->normals_m, nb); get(&t->colors_m, nb); get(&t->orig, (size_t)cap * sizeof(int));
    get(&t->tile_box, (size_t)mesh_tiles(cap) * 3 * sizeof(float4));
  };
  auto mask_set = [&](SceneStore* t, int cap) {
    const size_t nwords = (size_t)((mesh_tiles(cap) + 63) / 64), g3 = (size_t)kWorldGrid * kWorldGrid * kWorldGrid;
    get(&t->screen_masks, (size_t)mesh_screen_cells(cfg.width) * mesh_screen_cells(cfg.height) * nwords * 8);
    get(&t->world_masks, g3 * nwords * 8);
  };
  const bool grow = n > c->cap || !c->d_verts;
  const int cap = grow ? (n > 0 ? n : 1) : c->cap;
  if (grow) {    // (what the context already keeps for another family grows too: a later replace within capacity allocates nothing)
    const size_t nb = (size_t)cap * sizeof(float4);
    g->cap = cap;
    get(&g->verts, 3 * nb); get(&g->normals, nb); get(&g->colors, nb);
    if (q.records || o.records) get(&g->t.records, (size_t)cap * kRecordsPerTriangle * sizeof(float4));
    if (q.tiled || o.verts_m) tiled_set(&g->t, cap);
    if (q.masks || o.screen_masks) mask_set(&g->t, cap);
  } else {
    if (q.records && !o.records) get(&o.records, (size_t)cap * kRecordsPerTriangle * sizeof(float4));
    if (q.tiled && !o.verts_m) tiled_set(&o, cap);
    if (q.masks && !o.screen_masks) mask_set(&o, cap);
  }
  if (q.masks && !o.world_occ) get(&o.world_occ, (size_t)mesh_occ_words(kWorldGrid) * sizeof(unsigned int));
  if (q.heavy && !o.heavy_flags) {
    get(&o.heavy[0], (size_t)c->heavy_cap * 4); get(&o.heavy[1], (size_t)c->heavy_cap * 4); get(&o.heavy_flags, 2 * c->heavy_jobs_max * 4);
  }
  if (q.mesh_sched && !o.mesh_cost) {
    const size_t jobs = (size_t)((cfg.width + 15) / 16) * (size_t)((c->owned_rows + 15) / 16);
    // order list: up to four entries per block, + its length in the word behind it
    get(&o.mesh_cost, (jobs ? jobs : 1) * 4); get(&o.mesh_order, (4 * (jobs ? jobs : 1) + 1) * 4);
  }
  if (!ok) { set_error("hipMalloc failed: %s", hipGetErrorString(hipGetLastError())); free_growth(g); return RT_E_NOMEM; }
  if (device_tiles && q.tiled) {
    const int rc = ensure_bytes(&c->tile_scratch, tile_build_scratch_bytes(cap));
    if (rc != RT_OK) { free_growth(g); return rc; }
  }
  if (q.masks && !c->aux_stream &&
      (hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking) != hipSuccess ||
       hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
       hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess)) {
    set_error("stream/event creation failed"); free_growth(g); return RT_E_DEVICE;
  }
  return RT_OK;
}

// The grown buffers take the place of the old ones.  hipFree waits for whatever still uses what it frees.  From here to
// scene_select the context's working pointers are stale: the caller installs the new scene next, and nothing in between fails
// for a reason the caller could have (validation and allocation are behind it).
static void scene_commit(rt_ctx* c, SceneGrowth* g) {
  if (!g->cap) return;
  hipSetDevice(c->device);
  SceneStore& o = c->own;
  hipFree(c->d_verts); hipFree(c->d_normals); hipFree(c->d_colors);
  hipFree(o.records); hipFree(o.verts_m); hipFree(o.normals_m); hipFree(o.colors_m); hipFree(o.orig); hipFree(o.tile_box);
  hipFree(o.screen_masks); hipFree(o.world_masks);
  hipFree(c->d_qrecords); c->d_qrecords = nullptr;           // (the queries make theirs on demand, for the capacity)
  c->d_verts = g->verts; c->d_normals = g->normals; c->d_colors = g->colors;
  o.records = g->t.records;
  o.verts_m = g->t.verts_m; o.normals_m = g->t.normals_m; o.colors_m = g->t.colors_m; o.orig = g->t.orig; o.tile_box = g->t.tile_box;
  o.screen_masks = g->t.screen_masks; o.world_masks = g->t.world_masks;
  c->cap = g->cap;
  *g = SceneGrowth();
}

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

// Morton tiles on the device into d_orig (rt_tile_build.hip); rt_scene_refit follows
static int device_tiles(rt_ctx* c, const SceneSummary& sum, hipStream_t s) {
  if (launch_tile_build(c->d_verts, c->n, sum.lo, sum.hi, c->d_orig, c->tile_scratch.p, s) != 0) {
    set_error("tile build launch failed: %s", hipGetErrorString(hipGetLastError())); return RT_E_DEVICE;
  }
  return RT_OK;
}

static void refit(rt_ctx* c, hipStream_t s) {
  launch_scene_refit(c->d_verts, c->d_normals, c->d_colors, c->d_orig, c->n, c->d_verts_m, c->d_normals_m, c->d_colors_m,
                     c->d_tile_box, s);
}

// Host arrays (validated) into one single-device context; blocking.  replace: a scene of n triangles takes the place of
// the context's (scene_reserve / scene_commit are behind it); else n is the context's count.
static int scene_host_one(rt_ctx* c, const float* v4, const float* n4, const float* c4, int n, uint32_t flags,
                          const SceneSummary& sum, bool replace, bool first = false) {
  int rc = update_begin(c, c->stream);
  if (rc != RT_OK) return rc;
  if (replace) { rc = scene_switch(c, n, first, c->stream); if (rc != RT_OK) return rc; }
  const size_t nb = (size_t)n * sizeof(float4);
  if (n > 0) {
    HIP_TRY(hipMemcpyAsync(c->d_verts, v4, 3 * nb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_normals, n4, nb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_colors, c4, nb, hipMemcpyHostToDevice, c->stream));
  }
  if (c->d_verts_m) {
    if (flags & RT_UPDATE_DEVICE_TILES) {
      rc = device_tiles(c, sum, c->stream);
      if (rc != RT_OK) return rc;
      refit(c, c->stream);
      HIP_TRY(hipGetLastError());
    } else if (replace || (flags & RT_UPDATE_REORDER)) {
      rc = upload_tiled_scene(c, v4, n4, c4);
      if (rc != RT_OK) return rc;
    } else {
      refit(c, c->stream);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  update_state(c, sum);
  return RT_OK;
}

// Device arrays on device src_dev (validated) into one single-device context, enqueued on `s` (a stream of c->device);
// dc == nullptr: the colours stay (a pose)
static int scene_device_one(rt_ctx* c, const void* dv, const void* dn, const void* dc, int src_dev, int n, uint32_t flags,
                            hipStream_t s, const SceneSummary& sum, bool replace) {
  int rc = update_begin(c, s);
  if (rc != RT_OK) return rc;
  if (!c->ev_upd) HIP_TRY(hipEventCreateWithFlags(&c->ev_upd, hipEventDisableTiming));
  if (replace) { rc = scene_switch(c, n, false, s); if (rc != RT_OK) return rc; }
  const size_t nb = (size_t)n * sizeof(float4);
  if (src_dev == c->device) {
    HIP_TRY(hipMemcpyAsync(c->d_verts, dv, 3 * nb, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->d_normals, dn, nb, hipMemcpyDeviceToDevice, s));
    if (dc) HIP_TRY(hipMemcpyAsync(c->d_colors, dc, nb, hipMemcpyDeviceToDevice, s));
  } else {                                   // the other devices of a multi-device context: by peer copy, as the bands
    HIP_TRY(hipMemcpyPeerAsync(c->d_verts, c->device, dv, src_dev, 3 * nb, s));
    HIP_TRY(hipMemcpyPeerAsync(c->d_normals, c->device, dn, src_dev, nb, s));
    if (dc) HIP_TRY(hipMemcpyPeerAsync(c->d_colors, c->device, dc, src_dev, nb, s));
  }
  if (c->d_verts_m) {
    if (replace || (flags & RT_UPDATE_DEVICE_TILES)) { rc = device_tiles(c, sum, s); if (rc != RT_OK) return rc; }
    refit(c, s);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(c->ev_upd, s));
  c->upd_pending = true;
  update_state(c, sum);
  return RT_OK;
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
      const std::string msg = g_last_error;
      for (size_t j = 0; j < i; ++j) { hipSetDevice(ks[j]->device); free_growth(&grown[j]); }
      g_last_error = msg;
      return rc;
    }
  }
  for (size_t i = 0; i < ks.size(); ++i) scene_commit(ks[i], &grown[i]);
  return RT_OK;
}

// What a multi-device handle itself reports of the scene
static void parent_follows(rt_ctx* c) {
  if (!c->kids.empty()) { c->n = c->kids[0]->n; c->cap = c->kids[0]->cap; c->n_shadow = c->kids[0]->n_shadow; }
}

static int scene_first(rt_ctx* c, const float* v4, const float* n4, const float* c4, int n) {
  SceneGrowth g;
  int rc = scene_reserve(c, n, false, &g);
  if (rc != RT_OK) return rc;
  scene_commit(c, &g);
  SceneSummary sum;
  sum.n_shadow = count_shadow_casters(c4, n);
  if (scene_needs(c, n).masks) vertex_box(v4, n, sum.lo, sum.hi);
  return scene_host_one(c, v4, n4, c4, n, 0, sum, true, true);
}

static int replace_host_all(rt_ctx* c, const float* v4, const float* n4, const float* c4, int n, uint32_t flags, const SceneSummary& sum) {
  int rc = scene_reserve_all(c, n, (flags & RT_UPDATE_DEVICE_TILES) != 0);
  if (rc != RT_OK) return rc;
  for (rt_ctx* k : device_ctxs(c)) {
    rc = scene_host_one(k, v4, n4, c4, n, flags, sum, true);
    if (rc != RT_OK) return rc;
  }
  parent_follows(c);
  return RT_OK;
}

static int update_host_all(rt_ctx* c, const float* v4, const float* n4, const float* c4, int n, uint32_t flags, const SceneSummary& sum) {
  for (rt_ctx* k : device_ctxs(c)) {
    int rc = RT_OK;
    if ((flags & RT_UPDATE_DEVICE_TILES) && k->d_verts_m) {
      HIP_TRY(hipSetDevice(k->device));
      rc = ensure_bytes(&k->tile_scratch, tile_build_scratch_bytes(k->cap));
    }
    if (rc == RT_OK) rc = scene_host_one(k, v4, n4, c4, n, flags, sum, false);
    if (rc != RT_OK) return rc;
  }
  return RT_OK;
}

static const uint32_t kUpdateFlags = RT_UPDATE_REORDER | RT_UPDATE_DEVICE_TILES;

static int check_scene_flags(uint32_t flags, const char* fn) {
  if (flags & ~kUpdateFlags) { set_error("%s: unknown flags 0x%x", fn, flags); return RT_E_INVALID; }
  if ((flags & kUpdateFlags) == kUpdateFlags) {
    set_error("%s: RT_UPDATE_REORDER (host tiles) and RT_UPDATE_DEVICE_TILES exclude each other", fn); return RT_E_INVALID;
  }
  return RT_OK;
}

static int check_update_args(const rt_ctx* c, const void* v, const void* nr, const void* col, int32_t n, uint32_t flags) {
  if (!c) { set_error("NULL context"); return RT_E_INVALID; }
  if (n != c->n) { set_error("rt_update_scene: n = %d, but the context holds %d triangles", n, c->n); return RT_E_INVALID; }
  if (n > 0 && (!v || !nr || !col)) { set_error("scene arrays missing"); return RT_E_INVALID; }
  return check_scene_flags(flags, "rt_update_scene");
}

static int check_replace_args(const rt_ctx* c, const void* v, const void* nr, const void* col, int32_t n, uint32_t flags) {
  if (!c) { set_error("rt_replace_scene: NULL context"); return RT_E_INVALID; }
  if (!v || !nr || !col) { set_error("rt_replace_scene: scene arrays missing (NULL)"); return RT_E_INVALID; }
  if (n <= 0) { set_error("rt_replace_scene: n_new = %d, but a scene has at least one triangle", n); return RT_E_INVALID; }
  const int rc = check_scene_flags(flags, "rt_replace_scene");
  if (rc != RT_OK) return rc;
  if (n > 4000000) { set_error("triangle list of %d exceeds the supported maximum of 4000000", n); return RT_E_UNSUPPORTED; }
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
  if (!c->d_check) HIP_TRY(hipMalloc(&c->d_check, 8 * sizeof(unsigned int)));
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

// Device arrays into every device of the handle: a single device on the caller's stream; several devices each on its own
// stream after the caller's earlier work, copying from devices[0], and the caller's stream passes only when all have it
static int scene_device_all(rt_ctx* c, const void* dv, const void* dn, const void* dc, int n, uint32_t flags, hipStream_t s,
                            const SceneSummary& sum, bool replace) {
  if (c->kids.empty()) return scene_device_one(c, dv, dn, dc, c->device, n, flags, s, sum, replace);
  HIP_TRY(hipEventRecord(c->ev_go, s));
  for (rt_ctx* k : c->kids) {
    HIP_TRY(hipSetDevice(k->device));
    HIP_TRY(hipStreamWaitEvent(k->stream, c->ev_go, 0));
    const int rc = scene_device_one(k, dv, dn, dc, c->device, n, flags, k->stream, sum, replace);
    if (rc != RT_OK) return rc;
  }
  HIP_TRY(hipSetDevice(c->device));
  for (rt_ctx* k : c->kids) HIP_TRY(hipStreamWaitEvent(s, k->ev_upd, 0));
  return RT_OK;
}

// The scene of a device entry through host memory (RT_UPDATE_REORDER: the tiles are sorted on the host)
struct HostScene {
  std::vector<float> v, nr, col;
};

static int stage_to_host(const void* dv, const void* dn, const void* dc, int n, hipStream_t s, HostScene* h) {
  h->v.resize((size_t)n * 12); h->nr.resize((size_t)n * 4); h->col.resize((size_t)n * 4);
  HIP_TRY(hipMemcpyAsync(h->v.data(), dv, h->v.size() * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(h->nr.data(), dn, h->nr.size() * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(h->col.data(), dc, h->col.size() * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return RT_OK;
}

// A same-count scene in device memory on the handle's device that has passed device_check (the caller's arrays, or the
// staging scene a pose has written; dc == nullptr: the colours stay) into every device of the handle, behind stream s
static int update_from_device(rt_ctx* c, const void* dv, const void* dn, const void* dc, int n, uint32_t flags, hipStream_t s,
                              const SceneSummary& sum) {
  if (flags & RT_UPDATE_REORDER) {             // the tiles are sorted on the host: stage the scene through it
    HostScene h;
    const int rc = stage_to_host(dv, dn, dc ? dc : lead_ctx(c)->d_colors, n, s, &h);
    if (rc != RT_OK) return rc;
    return update_host_all(c, h.v.data(), h.nr.data(), h.col.data(), n, flags, sum);
  }
  if (flags & RT_UPDATE_DEVICE_TILES)
    for (rt_ctx* k : device_ctxs(c))
      if (k->d_verts_m) {
        HIP_TRY(hipSetDevice(k->device));
        const int rc = ensure_bytes(&k->tile_scratch, tile_build_scratch_bytes(k->cap));
        if (rc != RT_OK) return rc;
      }
  return scene_device_all(c, dv, dn, dc, n, flags, s, sum, false);
}

// ---- rigid objects (rt_set_objects / rt_pose_objects*): DESIGN.md 4.2b -------------------------------------------------
// The table and the rest pose live on the context that poses (lead_ctx).  Nothing here runs for a context without a table.
static void drop_objects(rt_ctx* c) {
  rt_ctx* L = lead_ctx(c);
  L->nobj = 0;
  if (!L->d_rest_verts && !L->d_rest_normals && !L->d_object_of) return;
  DeviceGuard guard;
  hipSetDevice(L->device);
  hipFree(L->d_rest_verts); hipFree(L->d_rest_normals); hipFree(L->d_object_of);   // (hipFree waits for a pose still reading them)
  L->d_rest_verts = L->d_rest_normals = nullptr; L->d_object_of = nullptr;
}

static int check_pose_args(rt_ctx* c, const void* xforms, uint32_t flags, const char* fn) {
  if (!c) { set_error("%s: NULL context", fn); return RT_E_INVALID; }
  if (!xforms) { set_error("%s: the matrices are missing (NULL)", fn); return RT_E_INVALID; }
  const int rc = check_scene_flags(flags, fn);
  if (rc != RT_OK) return rc;
  if (lead_ctx(c)->nobj == 0) {
    set_error("%s: the context has no object table (rt_set_objects first; a scene update or replace drops it)", fn);
    return RT_E_INVALID;
  }
  return RT_OK;
}

// The rest pose posed by the matrices at d_xforms12 (device memory of the lead device) into the staging scene, on s, and
// from there into the context as a device update: the check runs on the staging scene, before anything live is written
static int pose_from_device(rt_ctx* c, const void* d_xforms12, uint32_t flags, hipStream_t s) {
  rt_ctx* L = lead_ctx(c);
  HIP_TRY(hipSetDevice(L->device));
  const size_t nb = (size_t)L->cap * sizeof(float4);
  int rc = ensure_bytes(&L->pose_verts, 3 * nb);
  if (rc == RT_OK) rc = ensure_bytes(&L->pose_normals, nb);
  if (rc != RT_OK) return rc;
  // the staging scene may still be the source of the previous pose's copies, on whichever streams they run
  for (rt_ctx* k : device_ctxs(c)) HIP_TRY(wait_scene(k, s));
  launch_pose(L->d_rest_verts, L->d_rest_normals, L->d_object_of, (const float*)d_xforms12, L->n, (float4*)L->pose_verts.p,
              (float4*)L->pose_normals.p, s);
  HIP_TRY(hipGetLastError());
  SceneSummary sum;
  rc = device_check(c, L->pose_verts.p, L->d_colors, L->n, s, &sum);
  if (rc != RT_OK) return rc;
  return update_from_device(c, L->pose_verts.p, L->pose_normals.p, nullptr, L->n, flags, s, sum);
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
  HIP_TRY(hipSetDevice(L->device));
  const size_t nb = (size_t)n * sizeof(float4);
  if (!L->d_rest_verts &&      // (a table in force has buffers of this n: whatever changes n drops the table)
      (hipMalloc(&L->d_rest_verts, 3 * nb) != hipSuccess || hipMalloc(&L->d_rest_normals, nb) != hipSuccess ||
       hipMalloc(&L->d_object_of, (size_t)n * sizeof(unsigned short)) != hipSuccess)) {
    set_error("hipMalloc failed: %s", hipGetErrorString(hipGetLastError()));
    drop_objects(c);
    return RT_E_NOMEM;
  }
  // the snapshot waits for whatever still writes the scene, and a pose still reading the old rest pose (an update's event)
  int rc = update_begin(L, L->stream);
  if (rc == RT_OK &&
      (hipMemcpyAsync(L->d_rest_verts, L->d_verts, 3 * nb, hipMemcpyDeviceToDevice, L->stream) != hipSuccess ||
       hipMemcpyAsync(L->d_rest_normals, L->d_normals, nb, hipMemcpyDeviceToDevice, L->stream) != hipSuccess ||
       hipMemcpyAsync(L->d_object_of, object_of.data(), (size_t)n * sizeof(unsigned short), hipMemcpyHostToDevice, L->stream) != hipSuccess ||
       hipStreamSynchronize(L->stream) != hipSuccess)) {
    set_error("rt_set_objects: snapshot failed: %s", hipGetErrorString(hipGetLastError())); rc = RT_E_DEVICE;
  }
  if (rc != RT_OK) { const std::string msg = g_last_error; drop_objects(c); g_last_error = msg; return rc; }
  L->nobj = nobj;
  return RT_OK;
}

int rt_pose_objects(rt_ctx* c, const float* xforms12, uint32_t flags) {
  int rc = check_pose_args(c, xforms12, flags, "rt_pose_objects");
  if (rc != RT_OK) return rc;
  rt_ctx* L = lead_ctx(c);
  DeviceGuard guard;
  HIP_TRY(hipSetDevice(L->device));
  const size_t bytes = (size_t)L->nobj * 12 * sizeof(float);
  rc = ensure_bytes(&L->pose_xforms, bytes);     // (only this blocking entry uses the buffer: nothing can still be reading it)
  if (rc != RT_OK) return rc;
  HIP_TRY(hipMemcpyAsync(L->pose_xforms.p, xforms12, bytes, hipMemcpyHostToDevice, c->stream));
  rc = pose_from_device(c, L->pose_xforms.p, flags, c->stream);
  if (rc != RT_OK) { const std::string msg = g_last_error; hipStreamSynchronize(c->stream); (void)hipGetLastError(); g_last_error = msg; return rc; }
  HIP_TRY(hipStreamSynchronize(c->stream));      // (the stream of a multi-device handle has waited for every device)
  return RT_OK;
}

int rt_pose_objects_device(rt_ctx* c, const void* d_xforms12, uint32_t flags, void* hip_stream) {
  const int rc = check_pose_args(c, d_xforms12, flags, "rt_pose_objects_device");
  if (rc != RT_OK) return rc;
  DeviceGuard guard;
  return pose_from_device(c, d_xforms12, flags, (hipStream_t)hip_stream);
}

int rt_debug_object_count(rt_ctx* c, int32_t* out) {
  if (!c || !out) { set_error("rt_debug_object_count: NULL argument"); return RT_E_INVALID; }
  *out = lead_ctx(c)->nobj;
  return RT_OK;
}

int rt_update_scene(rt_ctx* c, const float* vertices4, const float* normals4, const float* colors4, int32_t n, uint32_t flags) {
  int rc = check_update_args(c, vertices4, normals4, colors4, n, flags);
  if (rc != RT_OK) return rc;
  rc = validate_vertices(vertices4, n);        // once, before any device is touched
  if (rc != RT_OK) return rc;
  if (n == 0) return RT_OK;
  SceneSummary sum;
  sum.n_shadow = count_shadow_casters(colors4, n);
  vertex_box(vertices4, n, sum.lo, sum.hi);
  DeviceGuard guard;
  drop_objects(c);                             // the scene behind the rest pose changes
  return update_host_all(c, vertices4, normals4, colors4, n, flags, sum);
}

int rt_update_scene_device(rt_ctx* c, const void* d_vertices4, const void* d_normals4, const void* d_colors4, int32_t n,
                           uint32_t flags, void* hip_stream) {
  int rc = check_update_args(c, d_vertices4, d_normals4, d_colors4, n, flags);
  if (rc != RT_OK) return rc;
  if (n == 0) return RT_OK;
  DeviceGuard guard;
  const hipStream_t s = (hipStream_t)hip_stream;
  // first pass: check the bound and reduce n_shadow and the box; the live buffers stay untouched until it has passed
  SceneSummary sum;
  rc = device_check(c, d_vertices4, d_colors4, n, s, &sum);
  if (rc != RT_OK) return rc;
  drop_objects(c);
  return update_from_device(c, d_vertices4, d_normals4, d_colors4, n, flags, s, sum);
}

int rt_replace_scene(rt_ctx* c, const float* vertices4, const float* normals4, const float* colors4, int32_t n_new, uint32_t flags) {
  int rc = check_replace_args(c, vertices4, normals4, colors4, n_new, flags);
  if (rc != RT_OK) return rc;
  rc = validate_vertices(vertices4, n_new);    // once, before any device is touched
  if (rc != RT_OK) return rc;
  SceneSummary sum;
  sum.n_shadow = count_shadow_casters(colors4, n_new);
  vertex_box(vertices4, n_new, sum.lo, sum.hi);
  DeviceGuard guard;
  drop_objects(c);
  return replace_host_all(c, vertices4, normals4, colors4, n_new, flags, sum);
}

int rt_replace_scene_device(rt_ctx* c, const void* d_vertices4, const void* d_normals4, const void* d_colors4, int32_t n_new,
                            uint32_t flags, void* hip_stream) {
  int rc = check_replace_args(c, d_vertices4, d_normals4, d_colors4, n_new, flags);
  if (rc != RT_OK) return rc;
  DeviceGuard guard;
  const hipStream_t s = (hipStream_t)hip_stream;
  SceneSummary sum;
  rc = device_check(c, d_vertices4, d_colors4, n_new, s, &sum);
  if (rc != RT_OK) return rc;
  drop_objects(c);
  if (flags & RT_UPDATE_REORDER) {             // host tiles (kd or Morton by the context's tuning): through the host
    HostScene h;
    rc = stage_to_host(d_vertices4, d_normals4, d_colors4, n_new, s, &h);
    if (rc != RT_OK) return rc;
    return replace_host_all(c, h.v.data(), h.nr.data(), h.col.data(), n_new, flags, sum);
  }
  rc = scene_reserve_all(c, n_new, true);
  if (rc != RT_OK) return rc;
  rc = scene_device_all(c, d_vertices4, d_normals4, d_colors4, n_new, flags, s, sum, true);
  parent_follows(c);
  return rc;
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

}  // extern "C"

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
    const std::string msg = g_last_error;
    for (size_t k = 0; k < nk; ++k)
      if (launched[k]) { hipSetDevice(p->kids[k]->device); hipStreamSynchronize(p->kids[k]->stream); }
    (void)hipGetLastError();
    g_last_error = msg;
    return rc;
  };
  // pass 1: every device's frame is launched before any band is delivered.  (Delivering inside this loop made the host
  // thread wait for device k's kernel and copy — a device-to-pageable-host copy blocks — before it launched device k+1:
  // the devices then ran one after another.)
  for (size_t k = 0; k < nk; ++k) {
    rt_ctx* c = p->kids[k];
    if (c->owned_rows == 0) continue;
    if (hipSetDevice(c->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", c->device); return fail(RT_E_DEVICE); }
    if (want_rgb && !c->d_rgb && hipMalloc(&c->d_rgb, (size_t)c->owned_rows * W * sizeof(float4)) != hipSuccess) {
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
    HIP_TRY(hipMalloc(&c->d_rgb, (px ? px : 1) * sizeof(float4)));
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

int rt_count_work(rt_ctx* c, const float rot[12], const float cam[3], const float light[3], float focal, rt_work* out) {
  if (!c || !out || !rot || !cam || !light) { set_error("NULL argument"); return RT_E_INVALID; }
  memset(out, 0, sizeof *out);
  DeviceGuard guard;
  if (!c->kids.empty()) {
    for (rt_ctx* k : c->kids) {
      rt_work w;
      const int rc = rt_count_work(k, rot, cam, light, focal, &w);
      if (rc != RT_OK) return rc;
      for (size_t q = 0; q < sizeof(rt_work) / 8; ++q) ((uint64_t*)out)[q] += ((const uint64_t*)&w)[q];
    }
    return RT_OK;
  }
  if (c->owned_rows == 0) return RT_OK;
  FrameParams P;
  fill_params(c, rot, cam, light, focal, &P);
  P.counters = c->d_counters;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(wait_aov(c, c->stream));
  HIP_TRY(wait_scene(c, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_counters, 0, sizeof(rt_work), c->stream));
  launch_generic(P, true, c->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, c->d_counters, sizeof(rt_work), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RT_OK;
}

int rt_count_executed(rt_ctx* c, const float rot[12], const float cam[3], const float light[3], float focal, uint64_t out[8]) {
  if (!c || !out || !rot || !cam || !light) { set_error("NULL argument"); return RT_E_INVALID; }
  memset(out, 0, 8 * sizeof(uint64_t));
  DeviceGuard guard;
  if (!c->kids.empty()) {
    for (rt_ctx* k : c->kids) {
      uint64_t w[8];
      const int rc = rt_count_executed(k, rot, cam, light, focal, w);
      if (rc != RT_OK) return rc;
      for (int q = 0; q < 8; ++q) out[q] += w[q];
    }
    return RT_OK;
  }
  if (c->owned_rows == 0) return RT_OK;
  FrameParams P;
  fill_params(c, rot, cam, light, focal, &P);
  const bool generic = (c->cfg.flags & RT_FLAG_GENERIC_KERNEL) != 0;
  const bool mesh = !generic && !wave_kernel_supports(P) && !(c->cfg.flags & RT_FLAG_NO_CULL) && mesh_kernel_supports(P);
  if (generic || (!wave_kernel_supports(P) && !mesh) || (!mesh && P.S > 64)) {
    set_error("rt_count_executed: this configuration runs on the generic kernel, whose executed work is rt_count_work");
    return RT_E_UNSUPPORTED;
  }
  if (!mesh && P.aa_x * P.aa_y > 64) {
    set_error("rt_count_executed: more than 64 AA samples per pixel run on the wave kernel's chunked build, which has no counting build");
    return RT_E_UNSUPPORTED;
  }
  P.counters = c->d_counters;
  HIP_TRY(hipSetDevice(c->device));
  if (c->timed) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev1, 0));
  HIP_TRY(wait_aov(c, c->stream));
  HIP_TRY(wait_scene(c, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_counters, 0, sizeof(rt_work), c->stream));
  if (mesh) { use_tiled_scene(c, &P); launch_stage_records(P, c->stream); launch_mesh(P, true, c->tune.phase_profile, c->stream, nullptr, nullptr, nullptr); }
  else if (c->tune.phase_profile) launch_wave_prof(P, c->stream);   // diagnostic: s_memtime per phase
  else launch_wave(P, !(c->cfg.flags & RT_FLAG_NO_CULL), true, c->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, c->d_counters, sizeof(rt_work), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RT_OK;
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
  float *d_rays = nullptr, *d_r2 = nullptr, *d_out = nullptr;
  int* d_tri = nullptr;
  int rc = RT_OK;
  if (hipMalloc(&d_rays, (size_t)nray * 24) != hipSuccess || hipMalloc(&d_tri, (size_t)nray * 4) != hipSuccess ||
      (radius_sq && hipMalloc(&d_r2, (size_t)nray * 4) != hipSuccess) || (out10 && hipMalloc(&d_out, (size_t)nray * 40) != hipSuccess)) {
    set_error("hipMalloc failed: %s", hipGetErrorString(hipGetLastError())); rc = RT_E_NOMEM;
  }
  auto ok = [&](hipError_t e, const char* opn) {
    if (rc == RT_OK && e != hipSuccess) { set_error("%s failed: %s", opn, hipGetErrorString(e)); rc = RT_E_DEVICE; }
  };
  if (rc == RT_OK) {
    if (c->timed) ok(hipStreamWaitEvent(c->stream, c->ev1, 0), "hipStreamWaitEvent");
    ok(wait_aov(c, c->stream), "hipStreamWaitEvent");
    ok(wait_scene(c, c->stream), "hipStreamWaitEvent");
    ok(hipMemcpyAsync(d_rays, rays6, (size_t)nray * 24, hipMemcpyHostToDevice, c->stream), "ray upload");
    if (radius_sq) ok(hipMemcpyAsync(d_r2, radius_sq, (size_t)nray * 4, hipMemcpyHostToDevice, c->stream), "ray upload");
    if (d_out) ok(hipMemsetAsync(d_out, 0, (size_t)nray * 40, c->stream), "hipMemsetAsync");
    if (rc == RT_OK) {
      if (generic_needs_records(c->n)) launch_stage_records(P, c->stream);
      launch_trace_rays(P, what, d_rays, d_r2, (long)nray, d_tri, d_out, c->stream);
      ok(hipGetLastError(), "trace kernel launch");
    }
    ok(hipMemcpyAsync(out_tri, d_tri, (size_t)nray * 4, hipMemcpyDeviceToHost, c->stream), "read-back");
    if (out10 && what == RT_TRACE_CLOSEST_HIT) ok(hipMemcpyAsync(out10, d_out, (size_t)nray * 40, hipMemcpyDeviceToHost, c->stream), "read-back");
    ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  }
  hipFree(d_rays); hipFree(d_r2); hipFree(d_out); hipFree(d_tri);
  return rc;
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

void rt_destroy(rt_ctx* c) {
  if (!c) return;
  DeviceGuard guard;
  for (rt_ctx* k : c->kids) rt_destroy(k);
  hipSetDevice(c->device);
  if (c->stream) { hipStreamSynchronize(c->stream); hipStreamDestroy(c->stream); }
  if (c->ev0) hipEventDestroy(c->ev0);
  if (c->ev1) hipEventDestroy(c->ev1);
  if (c->aux_stream) { hipStreamSynchronize(c->aux_stream); hipStreamDestroy(c->aux_stream); }
  if (c->ev_fork) hipEventDestroy(c->ev_fork);
  if (c->ev_join) hipEventDestroy(c->ev_join);
  if (c->ev_go) hipEventDestroy(c->ev_go);
  if (c->ev_done) hipEventDestroy(c->ev_done);
  if (c->ev_upd) hipEventDestroy(c->ev_upd);
  for (SideCall* k : {&c->query, &c->shade, &c->rad, &c->aov}) {     // no call of any family may still be running
    if (k->ev) { hipEventSynchronize(k->ev); hipEventDestroy(k->ev); }
    hipFree(k->d_stats); hipFree(k->io.p);
  }
  hipFree(c->d_qrecords); hipFree(c->rrec.p);
  hipFree(c->d_verts); hipFree(c->d_normals); hipFree(c->d_colors);
  hipFree(c->d_argb); hipFree(c->d_rgb); hipFree(c->d_counters); hipFree(c->d_jobctr);
  // (what a replaced scene may drop and regain is owned by the store; the working pointers are aliases)
  const SceneStore& o = c->own;
  hipFree(o.records); hipFree(o.screen_masks); hipFree(o.world_masks); hipFree(o.world_occ);
  if (c->reg_host && c->reg_owner) hipHostUnregister(c->reg_host);
  hipFree(o.heavy[0]); hipFree(o.heavy[1]); hipFree(o.heavy_flags); hipFree(c->d_timeline);
  hipFree(o.mesh_cost); hipFree(o.mesh_order); hipFree(c->d_spheres);
  hipFree(o.verts_m); hipFree(o.normals_m); hipFree(o.colors_m); hipFree(o.orig); hipFree(o.tile_box);
  hipFree(c->d_check); hipFree(c->tile_scratch.p);
  hipFree(c->d_rest_verts); hipFree(c->d_rest_normals); hipFree(c->d_object_of);
  hipFree(c->pose_verts.p); hipFree(c->pose_normals.p); hipFree(c->pose_xforms.p);
  delete c;
}

}  // extern "C"
