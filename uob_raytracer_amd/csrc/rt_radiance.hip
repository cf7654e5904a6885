// rt_radiance.hip — the frame's full colour for caller rays (rt_radiance_rays / rt_radiance_rays_device, include/uob_rt.h):
// the closest hit of each ray, the reflect / refract bounce loop of secondary_light (kernels.cl:342-365) with the context's
// max_bounces, and the two colour rules of draw (kernels.cl:416-423) over the soft-shadowed direct light of the first
// diffuse surface reached, bit for bit.  Two kernels on one stream, no host round trip between them:
//   A. rt_radiance_trace, lane = ray.  Persistent waves pull runs of 64-ray groups from a queue head behind the counters.
//      The first hit is tile_walk<false> (rt_tiles.h, the walk of rt_trace_rays' closest-hit queries; BOXES = false for
//      contexts without a tiled copy) finished from the scene arrays (finish_hit), then closest_spheres.  The bounce loop is wave-wide:
//      while any lane is on a mirror or glass surface and b < max_bounces, those lanes take reflect_ray / refract_ray
//      (rt_trace.h; the medium is carried in the lane's ray) and the wave walks again with only them active — the walk is
//      one call site inside the loop, iteration 0 being the caller's ray.  A ray that ends black (miss, or the loop ran
//      out) gets its zero colour here; a ray that reached a diffuse surface is appended to the context's record scratch:
//      ballot, popcount, one returning atomic per wave on the record count, which is also counter 2 of the call.
//        record = 3 float4: P | ray index + rule bit,  N | seed,  albedo.xyz
//   B. rt_radiance_shade, lane = (record, sample): shade_groups (rt_shade_body.h), rt_shade_points' own body — jump-table
//      generator, tile_walk<true>, shadow_spheres, the 0.0f * term summation rule — over the records, their count read from
//      device memory.  The record's first lane turns the light L into the colour, albedo * (0.5f + L) for a first hit and
//      (0.9f * (0.5f + L)) * albedo behind a bounce, and stores out_rgba4[ray index] itself.  A record whose term is 0 is not
//      traced: its light is +0 whatever its samples see, so the skip changes no bit.
// Both kernels pop their queue with queue_pop and leave their counters through flush_counters (rt_tiles.h): stage A in its own
// slots, stage B after renaming the three of the shade body's counters that a radiance call reports.
// Every skip of the walks is a certificate that the reference's test cannot accept; rays outside the certificates' domain
// (in_query_domain) — caller rays, bounce rays and sample rays alike — take every triangle.
// Compiled with -ffp-contract=off: see rt_math.h for the numerics contract.
#include "rt_host.h"
#include "rt_shade_body.h"

namespace uobrt {

namespace {

// Work counters of a call (rt_debug_radiance_stats), then the queue heads of the two kernels
enum { RD_RAYS, RD_BOUNCES, RD_POINTS, RD_SAMPLES, RD_CTILES, RD_CTESTS, RD_STESTS, RD_UNCULLED, RD_SLOTS = 8 };
constexpr int kRadHeadA = RD_SLOTS, kRadHeadB = RD_SLOTS + 1;
constexpr uint32_t kRuleBounce = 0x80000000u;   // record tag: the surface was reached through a bounce (ray indices are < 2^31)

// The records in, colours out
struct RadianceIO {
  const float4* __restrict__ records;
  float4* __restrict__ out_rgba;
  __device__ __forceinline__ bool trace_all() const { return false; }
  __device__ __forceinline__ void load(long k, Ray& pt, int& gid) const {
    const float4 a = records[3 * k], b = records[3 * k + 1];
    pt.P = xyz(a); pt.N = xyz(b);
    gid = __float_as_int(b.w);
  }
  __device__ __forceinline__ void store(long k, float light, int) const {
    const float4 a = records[3 * k], c = records[3 * k + 2];
    const uint32_t tag = __float_as_uint(a.w);
    const float l = 0.5f + light;                                 // indirect_light + direct, kernels.cl:354 / :421
    f3 col;
    if (tag & kRuleBounce) {
      const float s = 0.9f * l;
      col = mk(s * c.x, s * c.y, s * c.z);
    } else {
      col = mk(c.x * l, c.y * l, c.z * l);
    }
    out_rgba[tag & ~kRuleBounce] = make_float4(col.x, col.y, col.z, 1.0f);
  }
};

}  // namespace

// Stage A.  P: fill_params of the context (+ use_tiled_scene when BOXES).  rays = nray x (start, direction); seeds nullable
// (k & 0xFFFFFF); out_prim nullable; records: 3 * nray float4.  stats: radiance_stats_words() zeroed 64-bit words.
// (amdgpu_waves_per_eu(4): a lane carries its whole Ray — start, direction, hit, colour, medium — across the walk)
template <bool BOXES>
__global__ __launch_bounds__(64 * kShadeWaves) __attribute__((amdgpu_waves_per_eu(4)))
void rt_radiance_trace(const FrameParams P, const float* __restrict__ rays, const int* __restrict__ seeds, long nray,
                       float4* __restrict__ out_rgba, int* __restrict__ out_prim, float4* __restrict__ records,
                       unsigned long long* __restrict__ stats, int run) {
  __shared__ float4 s_tile[kShadeWaves][4 * kQTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long ngroups = (nray + 63) >> 6;
  unsigned int* const head = reinterpret_cast<unsigned int*>(stats + kRadHeadA);
  unsigned long long w[RD_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};   // (RD_POINTS is added to as the records are appended, below)
  unsigned long long n_bundle = 0;            // (the walk counts its candidate tiles; a radiance call does not report them)
  unsigned long long tests = 0;               // this lane's
  Work wk;                                    // (the counting slot of closest_spheres<false>: never written)
  for (;;) {
    const unsigned int g0 = queue_pop(head, lane);
    if ((long)g0 * run >= ngroups) break;
    for (int gr = 0; gr < run; ++gr) {
      const long g = (long)g0 * run + gr;
      if (g >= ngroups) break;
      const long k = g * 64 + lane;
      const bool act = k < nray;
      Ray ray;                                // starts in air: medium AIR, colour w = 1, no triangle
      ray.start = mk(0.f, 0.f, 0.f); ray.dir = ray.start; ray.P = ray.start; ray.N = ray.start;
      ray.tri = -1; ray.medium = RT_AIR;
      ray.col = make_float4(0.f, 0.f, 0.f, 1.0f);
      if (act) {
        ray.start = mk(rays[6 * k], rays[6 * k + 1], rays[6 * k + 2]);
        ray.dir = mk(rays[6 * k + 3], rays[6 * k + 4], rays[6 * k + 5]);
      }
      w[RD_RAYS] += __popcll(ballot(act));
      bool go = act;                          // the lane's ray is still to be traced
      bool emit = false, bounced = false;     // it ended on a diffuse surface (through a bounce)
      int prim = -1;                          // the first hit
      for (int it = 0;; ++it) {               // 0: the caller's ray; b + 1: bounce b of secondary_light
        TileHit h = no_hit();
        bool blocked = false;                 // (the any-hit slot of the shared walk: unused by closest hit)
        tile_walk<false, BOXES>(P, s_tile[wave], lane, go, ray.start, ray.dir, 0.0f, h, blocked, w[RD_UNCULLED], n_bundle, w[RD_CTILES], tests);
        if (go) {
          finish_hit(P, h, ray);
          float current_t = h.t;
          closest_spheres<false>(P, ray, current_t, wk);
          if (it == 0) prim = ray.tri;
          const bool specular = ray.col.w <= 0.0f;
          // kernels.cl:416-418 for the first hit (anything not specular is lit), :351 behind a bounce (w > 0 is lit)
          const bool lit = ray.tri != -1 && (it == 0 ? !specular : ray.col.w > 0.0f);
          emit = lit; bounced = it > 0;
          go = ray.tri != -1 && specular;     // (a miss leaves the bounce ray's own w = 1: the loop of :345 ends)
        }
        if (it >= P.bounces) break;
        const unsigned long long gm = ballot(go);
        if (gm == 0ull) break;
        w[RD_BOUNCES] += __popcll(gm);
        if (go) ray = (ray.col.w == 0.0f) ? reflect_ray(ray) : refract_ray(ray);
      }
      // the rays that reached a diffuse surface: one slot each, in lane order, from one atomic per wave
      const unsigned long long em = ballot(emit);
      unsigned int base = 0u;
      if (em != 0ull) {
        if (lane == 0) base = (unsigned int)atomicAdd(&stats[RD_POINTS], (unsigned long long)__popcll(em));
        base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
      }
      if (emit) {
        const long q = (long)base + __popcll(em & ((1ull << lane) - 1ull));
        const int gid = seeds ? seeds[k] : (int)(k & 0xFFFFFF);
        const uint32_t tag = (uint32_t)k | (bounced ? kRuleBounce : 0u);
        records[3 * q] = make_float4(ray.P.x, ray.P.y, ray.P.z, __uint_as_float(tag));
        records[3 * q + 1] = make_float4(ray.N.x, ray.N.y, ray.N.z, __int_as_float(gid));
        records[3 * q + 2] = make_float4(ray.col.x, ray.col.y, ray.col.z, 0.f);
      } else if (act) {
        out_rgba[k] = make_float4(0.f, 0.f, 0.f, prim != -1 ? 1.0f : 0.0f);
      }
      if (act && out_prim) out_prim[k] = prim;
    }
  }
  flush_counters(stats, w, RD_CTESTS, tests);
}

// Stage B.  P: the same, with the call's light.  The record count is stats[RD_POINTS] as stage A left it; the grid is sized
// for nray records, and the waves beyond the count find the queue empty.
// (waves per SIMD as rt_shade's, except the tiled MULTI instantiation: held at 5 it spills two vector registers)
template <bool BOXES, bool MULTI>
__global__ __launch_bounds__(64 * kShadeWaves) __attribute__((amdgpu_waves_per_eu(MULTI && !BOXES ? 5 : 4)))
void rt_radiance_shade(const FrameParams P, const float4* __restrict__ records, float4* __restrict__ out_rgba,
                       unsigned long long* stats) {
  __shared__ float4 s_tile[kShadeWaves][4 * kQTile];
  __shared__ uint32_t s_jump[kJumpWords];
  stage_shade_jump(s_jump, threadIdx.x, 64 * kShadeWaves);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long npoints = (long)stats[RD_POINTS];
  const int ppw = MULTI ? 1 : 64 / P.S;
  const int run = shade_run((npoints + ppw - 1) / ppw, (long)gridDim.x * kShadeWaves, BOXES);
  unsigned long long w[SH_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tests = 0, unculled = 0;
  const RadianceIO io{records, out_rgba};
  shade_groups<BOXES, MULTI>(P, io, npoints, stats + kRadHeadB, run, s_tile[wave], s_jump, lane, w, tests, unculled);
  // of the shade body's counters a radiance call reports three, under its own names
  unsigned long long r[RD_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
  r[RD_SAMPLES] = w[SH_RAYS]; r[RD_UNCULLED] = unculled;
  flush_counters(stats, r, RD_STESTS, tests);
}

template __global__ void rt_radiance_trace<false>(const FrameParams, const float*, const int*, long, float4*, int*, float4*, unsigned long long*, int);
template __global__ void rt_radiance_trace<true>(const FrameParams, const float*, const int*, long, float4*, int*, float4*, unsigned long long*, int);
template __global__ void rt_radiance_shade<false, false>(const FrameParams, const float4*, float4*, unsigned long long*);
template __global__ void rt_radiance_shade<false, true>(const FrameParams, const float4*, float4*, unsigned long long*);
template __global__ void rt_radiance_shade<true, false>(const FrameParams, const float4*, float4*, unsigned long long*);
template __global__ void rt_radiance_shade<true, true>(const FrameParams, const float4*, float4*, unsigned long long*);

int radiance_stats_words() { return RD_SLOTS + 2; }
size_t radiance_record_bytes(long nray) { return (size_t)nray * 3 * sizeof(float4); }

// P: fill_params of the context with the call's light (+ use_tiled_scene when tiled).  d_records: radiance_record_bytes(nray);
// stats: radiance_stats_words() zeroed 64-bit words.  Both kernels go to `stream`, B behind A.
void launch_radiance(const FrameParams& P, bool tiled, const float* d_rays6, const int* d_seeds, long nray, float4* d_rgba,
                     int* d_prim, float4* d_records, unsigned long long* stats, int cus, hipStream_t stream) {
  typedef void (*Trace)(const FrameParams, const float*, const int*, long, float4*, int*, float4*, unsigned long long*, int);
  typedef void (*Shade)(const FrameParams, const float4*, float4*, unsigned long long*);
  const bool multi = P.S >= 64;
  const Trace trace = tiled ? &rt_radiance_trace<true> : &rt_radiance_trace<false>;
  const Shade shade = tiled ? (multi ? &rt_radiance_shade<true, true> : &rt_radiance_shade<true, false>)
                            : (multi ? &rt_radiance_shade<false, true> : &rt_radiance_shade<false, false>);
  {
    const long ngroups = (nray + 63) / 64;
    const dim3 grid(grid_blocks((ngroups + kShadeWaves - 1) / kShadeWaves,
                                (long)cus * blocks_per_cu(reinterpret_cast<const void*>(trace), 64 * kShadeWaves)));
    const int run = shade_run(ngroups, (long)grid.x * kShadeWaves, tiled);
    hipLaunchKernelGGL(trace, grid, dim3(64 * kShadeWaves), 0, stream, P, d_rays6, d_seeds, nray, d_rgba, d_prim, d_records, stats, run);
  }
  {
    const int ppw = multi ? 1 : 64 / P.S;
    const long ngroups = (nray + ppw - 1) / ppw;                  // (at most: every ray a record)
    const dim3 grid(grid_blocks((ngroups + kShadeWaves - 1) / kShadeWaves,
                                (long)cus * blocks_per_cu(reinterpret_cast<const void*>(shade), 64 * kShadeWaves)));
    hipLaunchKernelGGL(shade, grid, dim3(64 * kShadeWaves), 0, stream, P, d_records, d_rgba, stats);
  }
}

}  // namespace uobrt
