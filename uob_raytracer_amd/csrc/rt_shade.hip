// rt_shade.hip — soft-shadowed direct light at caller points (rt_shade_points / rt_shade_points_device, include/uob_rt.h):
// one channel of the reference's direct_light (kernels.cl:313-340) for a point (intersect, intersect_normal) and the
// global_id that seeds its jitter stream, with the context's shadow_samples and light_spread, bit for bit.
//
// Persistent waves pull runs of groups of whole points from a queue head behind the counters (`run` consecutive groups per
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
#include "rt_tiles.h"

// rt_wave_common.h lets the compiler fuse the BOUNDS it defines; what follows is the reference's arithmetic again
#pragma clang fp contract(off)

namespace uobrt {

namespace {

constexpr int kShadeWaves = 4;              // waves per workgroup (independent after the table is staged)
// Work counters of a call (rt_debug_shade_stats), then the queue head
enum { SH_POINTS, SH_RAYS, SH_WAVES, SH_TILES, SH_BUNDLE_TILES, SH_TESTED_TILES, SH_TRI_TESTS, SH_SKIPPED, SH_SLOTS = 8 };

// A^(4 q) for q = 1 .. 16 as nibble tables: nib[q - 1][j][v] = A^(4 q) (v << 4 j), so A^(4 q) s is the XOR of 8 entries
constexpr int kJumpRows = 16, kJumpWords = kJumpRows * 8 * 16;
struct ShadeJumpTable { uint32_t nib[kJumpRows][8][16]; };
constexpr ShadeJumpTable make_shade_jump_table() {
  ShadeJumpTable t{};
  for (int j = 0; j < 8; ++j)
    for (int v = 0; v < 16; ++v) {
      uint32_t s = (uint32_t)v << (4 * j);
      for (int q = 0; q < kJumpRows; ++q) {
        s = xorshift_c(xorshift_c(xorshift_c(xorshift_c(s))));
        t.nib[q][j][v] = s;
      }
    }
  return t;
}
__constant__ const ShadeJumpTable kShadeJump = make_shade_jump_table();

// A^k s for k = 0 .. 64 (jump = the table in LDS)
__device__ __forceinline__ uint32_t rng_advance(const uint32_t* jump, uint32_t s, int k) {
  const int q = k >> 2;
  if (q > 0) {
    const uint32_t* row = jump + (q - 1) * 128;
    uint32_t acc = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc ^= row[16 * j + ((s >> (4 * j)) & 15u)];
    s = acc;
  }
  for (int r = k & 3; r > 0; --r) s = xorshift(s);
  return s;
}

}  // namespace

// P: fill_params of the context with the call's light (+ use_tiled_scene when BOXES).  points6 = npoints x (position,
// normal); seeds nullable (k & 0xFFFFFF); out_cnt nullable: then a point whose term is 0 is not traced (its light is +0
// whatever its samples see).  stats: shade_stats_words() zeroed 64-bit words.
template <bool BOXES, bool MULTI>
__global__ __launch_bounds__(64 * kShadeWaves) __attribute__((amdgpu_waves_per_eu(MULTI ? 5 : 4)))
void rt_shade(const FrameParams P, const float* __restrict__ points6,
                                                              const int* __restrict__ seeds, long npoints, float* __restrict__ out_light,
                                                              int* __restrict__ out_cnt, unsigned long long* __restrict__ stats, int run) {
  __shared__ float4 s_tile[kShadeWaves][4 * kQTile];
  __shared__ uint32_t s_jump[kJumpWords];
  for (int i = threadIdx.x; i < kJumpWords; i += 64 * kShadeWaves) s_jump[i] = reinterpret_cast<const uint32_t*>(&kShadeJump)[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int S = P.S;
  const int ppw = MULTI ? 1 : 64 / S;                         // whole points per wave
  const int smagic = (65536 + S - 1) / S;                     // lane / S == (lane * smagic) >> 16 for lane < 64 (FrameParams::aa_magic)
  const int passes = MULTI ? (S + 63) >> 6 : 1;               // 64-sample passes per point (MULTI: S >= 64, one point per wave)
  const long ngroups = (npoints + ppw - 1) / ppw;
  const f3 light = mk(P.light[0], P.light[1], P.light[2]);
  unsigned int* const head = reinterpret_cast<unsigned int*>(stats + SH_SLOTS);
  unsigned long long w[SH_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tests = 0;
  unsigned long long unculled = 0;            // (tile_walk counts the rays outside the domain; a shade call does not report them)
  Work wk;                                    // (the counting slot of shadow_spheres<false>: never written)
  for (;;) {
    unsigned int g0 = 0u;
    if (lane == 0) g0 = atomicAdd(head, 1u);
    g0 = (unsigned int)__builtin_amdgcn_readfirstlane((int)g0);
    if ((long)g0 * run >= ngroups) break;
    for (int gr = 0; gr < run; ++gr) {
      const long g = (long)g0 * run + gr;
      if (g >= ngroups) break;
      // this lane's point of the group and its sample of the pass.  (From an opaque copy of the lane id, here and again after
      // the walk: hoisted out of the loops, pl, si, k and the segment mask are six registers held across the walk, which is
      // what decides between 4 and 5 waves per SIMD.)
      const int la = opaque(lane);
      const int pl = MULTI ? 0 : (la * smagic) >> 16, si = MULTI ? la : la - pl * S;
      const long k = g * ppw + pl;
      const bool have = pl < ppw && k < npoints;
      Ray pt;
      pt.P = mk(0.f, 0.f, 0.f); pt.N = pt.P;
      int gid = 0;
      if (have) {
        pt.P = mk(points6[6 * k], points6[6 * k + 1], points6[6 * k + 2]);
        pt.N = mk(points6[6 * k + 3], points6[6 * k + 4], points6[6 * k + 5]);
        gid = seeds ? seeds[k] : (int)(k & 0xFFFFFF);
      }
      const LightSetup l = light_setup(light, pt);
      const bool skip = have && !out_cnt && l.term == 0.0f;      // the frame's term == 0 skip
      w[SH_POINTS] += __popcll(ballot(have && si == 0));
      w[SH_SKIPPED] += __popcll(ballot(skip && si == 0));
      uint32_t r0 = rng_seed(gid, 0), r1 = rng_seed(gid, 1), r2 = rng_seed(gid, 2);     // the state after kernels.cl:319
      int unshadowed = 0;
      for (int pass = 0; pass < passes; ++pass) {
        const bool act = have && !skip && pass * 64 + si < S;
        if (ballot(act) == 0ull) break;                           // (every point of the group skipped)
        const f3 jit = mk(crush1(rng_advance(s_jump, r0, si + 1), P.spread), crush1(rng_advance(s_jump, r1, si + 1), P.spread),
                          crush1(rng_advance(s_jump, r2, si + 1), P.spread));
        const f3 d = l.dir + jit;
        TileHit h = no_hit();                                     // (the closest-hit slot of the shared walk: unused by SHADOW)
        bool blocked = false;
        w[SH_RAYS] += __popcll(ballot(act)); w[SH_WAVES] += 1;
        tile_walk<true, BOXES>(P, s_tile[wave], lane, act, l.start, d, l.radius_sq, h, blocked, unculled, w[SH_BUNDLE_TILES],
                               w[SH_TESTED_TILES], tests);
        const bool lit = act && !blocked && !shadow_spheres<false>(P, l.start, d, l.radius_sq, wk);
        const int lb = opaque(lane);
        const int plb = MULTI ? 0 : (lb * smagic) >> 16;
        const unsigned long long seg = MULTI ? ~0ull : (((1ull << S) - 1ull) << (plb < ppw ? plb * S : 0));   // the point's lanes
        unshadowed += __popcll(ballot(lit) & seg);
        if (pass + 1 < passes) { r0 = rng_advance(s_jump, r0, 64); r1 = rng_advance(s_jump, r1, 64); r2 = rng_advance(s_jump, r2, 64); }
      }
      const int lc = opaque(lane);
      const int plc = MULTI ? 0 : (lc * smagic) >> 16;
      const long kc = g * ppw + plc;
      if (plc < ppw && kc < npoints && (MULTI ? lc : lc - plc * S) == 0) {      // the point's first lane
        float total = 0.0f;
        if (unshadowed < S) total += 0.0f * l.term;               // a blocked sample adds 0*term (NaN/inf-faithful)
#pragma unroll 4
        for (int i = 0; i < unshadowed; ++i) total += l.term;
        out_light[kc] = div_count(total, S, P.inv_S);
        if (out_cnt) out_cnt[kc] = unshadowed;
      }
    }
  }
  const unsigned long long all_tests = wave_sum(tests);
  if (lane == 0) {
    w[SH_TRI_TESTS] = all_tests;
    for (int q = 0; q < SH_SLOTS; ++q)
      if (w[q]) atomicAdd(&stats[q], w[q]);
  }
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
  // resident workgroups per CU (the persistent grid), asked of the current device at every launch: nothing is cached across
  // contexts, devices or threads
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kernel), 64 * kShadeWaves, 0) != hipSuccess || per_cu < 1)
    per_cu = 2;
  const int ppw = multi ? 1 : 64 / P.S;
  const long ngroups = (npoints + ppw - 1) / ppw;
  const long want = (ngroups + kShadeWaves - 1) / kShadeWaves;
  const long full = (long)cus * per_cu;
  const dim3 grid((unsigned)(want < full ? want : full));
  // groups per hand-out, up to 32: a wave gets about 16 hand-outs without a tiled copy, where the groups cost much the same,
  // and about 64 on a mesh, where a group on the mesh costs many times a group on a wall (measured on the 100 026-triangle
  // scene, 2^18 points: runs of 3 took 59.8 ms, single groups 51.9)
  const long per = ngroups / ((long)grid.x * kShadeWaves * (tiled ? 64 : 16));
  const int run = (int)(per < 1 ? 1 : per > 32 ? 32 : per);
  hipLaunchKernelGGL(kernel, grid, dim3(64 * kShadeWaves), 0, stream, P, d_points6, d_seeds, npoints, d_light, d_cnt, stats, run);
}

}  // namespace uobrt
