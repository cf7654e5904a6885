// rt_shade.hip — soft-shadowed direct light at caller points (rt_shade_points / rt_shade_points_device, include/uob_rt.h):
// one channel of the reference's direct_light (kernels.cl:313-340) for a point (intersect, intersect_normal) and the
// global_id that seeds its jitter stream, with the context's shadow_samples and light_spread, bit for bit.
//
// Persistent waves pull runs of groups of whole points from a queue head behind the counters (queue_pop, rt_tiles.h; the
// counters leave through flush_counters, the grid is sized by blocks_per_cu and grid_blocks, rt_host.h; `run` consecutive groups per
// hand-out: a returning atomic on one word serves ~90 waves per microsecond, 2^20 single hand-outs alone would take 12 ms).
// lane = (point, sample): with S < 64 a wave takes floor(64 / S) points and the lanes beyond them idle (MULTI = false); with
// S >= 64 a wave holds one point, which takes ceil(S / 64) passes, and the counts accumulate (MULTI = true, held at 5 waves
// per SIMD; the other instantiation spills under that limit).  A wave never holds part of a point beside another point.
//   1. every lane builds its own sample ray in registers (light_setup of its point, the jitter of ITS sample): no ray exists
//      in memory.  The jitter stream is xorshift32, a linear map A of GF(2)^32; the state of sample i is A^(i + 1) applied to
//      the state after the seed step (rng_seed), reached as A^(4 q) through nibble tables in LDS (8 look-ups per component)
//      and at most 3 plain steps, instead of up to 64 dependent steps per lane;
//   2. the rays go through tile_walk<true> (rt_tiles.h), the walk of rt_trace_rays' in_shadow queries: bundle bound, per-lane
//      tile certificate, records in the wave's LDS with the per-triangle bundle bound (task_bound), any-hit with early
//      exit.  A point's samples are the tightest bundle there is (one start, directions within light_spread).  Contexts
//      without a tiled copy (n <= 64, RT_FLAG_GENERIC_KERNEL) take the same walk over runs of 64 triangles in scene order
//      (BOXES = false): no tile data, but task_bound still clears most of the triangles for a bundle this narrow;
//   3. the spheres (shadow_spheres) for the lanes still unblocked; ballot, popcount over the point's lane segment;
//   4. the point's first lane applies shade()'s summation rule (rt_wave_common.h): 0.0f * term once if a sample was blocked,
//      then term once per unblocked sample, then / S.
// Every skip of the walk is a certificate that the reference's test cannot accept; rays outside the certificates' domain
// (in_query_domain) take every triangle.  Compiled with -ffp-contract=off: see rt_math.h for the numerics contract.
#include "rt_host.h"
#include "rt_shade_body.h"

namespace uobrt {

namespace {

// The caller's points in, one light value (and, asked for, one count) per point out
struct ShadePointsIO {
  const float* __restrict__ points6;
  const int* __restrict__ seeds;
  float* __restrict__ out_light;
  int* __restrict__ out_cnt;
  __device__ __forceinline__ bool trace_all() const { return out_cnt != nullptr; }
  __device__ __forceinline__ void load(long k, Ray& pt, int& gid) const {
    pt.P = mk(points6[6 * k], points6[6 * k + 1], points6[6 * k + 2]);
    pt.N = mk(points6[6 * k + 3], points6[6 * k + 4], points6[6 * k + 5]);
    gid = seeds ? seeds[k] : (int)(k & 0xFFFFFF);
  }
  __device__ __forceinline__ void store(long k, float light, int unshadowed) const {
    out_light[k] = light;
    if (out_cnt) out_cnt[k] = unshadowed;
  }
};

}  // namespace

// P: fill_params of the context with the call's light (+ use_tiled_scene when BOXES).  points6 = npoints x (position,
// normal); seeds nullable (k & 0xFFFFFF); out_cnt nullable: then a point whose term is 0 is not traced (its light is +0
// whatever its samples see).  stats: shade_stats_words() zeroed 64-bit words.  The per-group body is shade_groups
// (rt_shade_body.h: tile_walk<true> and the summation rule), shared with rt_radiance.hip.
template <bool BOXES, bool MULTI>
__global__ __launch_bounds__(64 * kShadeWaves) __attribute__((amdgpu_waves_per_eu(MULTI ? 5 : 4)))
void rt_shade(const FrameParams P, const float* __restrict__ points6,
                                                              const int* __restrict__ seeds, long npoints, float* __restrict__ out_light,
                                                              int* __restrict__ out_cnt, unsigned long long* __restrict__ stats, int run) {
  __shared__ float4 s_tile[kShadeWaves][4 * kQTile];
  __shared__ uint32_t s_jump[kJumpWords];
  stage_shade_jump(s_jump, threadIdx.x, 64 * kShadeWaves);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long w[SH_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tests = 0;
  unsigned long long unculled = 0;            // (tile_walk counts the rays outside the domain; a shade call does not report them)
  const ShadePointsIO io{points6, seeds, out_light, out_cnt};
  shade_groups<BOXES, MULTI>(P, io, npoints, stats + SH_SLOTS, run, s_tile[wave], s_jump, lane, w,
                             tests, unculled);
  flush_counters(stats, w, SH_TRI_TESTS, tests);
}

template __global__ void rt_shade<false, false>(const FrameParams, const float*, const int*, long, float*, int*, unsigned long long*, int);
template __global__ void rt_shade<false, true>(const FrameParams, const float*, const int*, long, float*, int*, unsigned long long*, int);
template __global__ void rt_shade<true, false>(const FrameParams, const float*, const int*, long, float*, int*, unsigned long long*, int);
template __global__ void rt_shade<true, true>(const FrameParams, const float*, const int*, long, float*, int*, unsigned long long*, int);

int shade_stats_words() { return SH_SLOTS + 1; }

void launch_shade(const FrameParams& P, bool tiled, const float* d_points6, const int* d_seeds, long npoints, float* d_light,
                  int* d_cnt, unsigned long long* stats, int cus, hipStream_t stream) {
  typedef void (*Kernel)(const FrameParams, const float*, const int*, long, float*, int*, unsigned long long*, int);
  const bool multi = P.S >= 64;
  const Kernel kernel = tiled ? (multi ? &rt_shade<true, true> : &rt_shade<true, false>)
                              : (multi ? &rt_shade<false, true> : &rt_shade<false, false>);
  const int ppw = multi ? 1 : 64 / P.S;
  const long ngroups = (npoints + ppw - 1) / ppw;
  const dim3 grid(grid_blocks((ngroups + kShadeWaves - 1) / kShadeWaves,
                              (long)cus * blocks_per_cu(reinterpret_cast<const void*>(kernel), 64 * kShadeWaves)));
  const int run = shade_run(ngroups, (long)grid.x * kShadeWaves, tiled);
  hipLaunchKernelGGL(kernel, grid, dim3(64 * kShadeWaves), 0, stream, P, d_points6, d_seeds, npoints, d_light, d_cnt, stats, run);
}

}  // namespace uobrt
