// rt_shade_body.h — the per-group body of the direct-light kernels, shared by rt_shade_points (rt_shade.hip: the points are
// the caller's) and the second stage of rt_radiance_rays (rt_radiance.hip: the points are the records its first stage left,
// and the light becomes a colour).  Where the points come from and where the light goes is the IO policy's business:
//   bool trace_all()                         true: a point whose term is 0 is traced all the same (its sample count is wanted)
//   void load(long k, Ray& pt, int& gid)     point k: pt.P, pt.N and the global_id that seeds its jitter stream
//   void store(long k, float light, int unshadowed)     called by the point's first lane
// Include after rt_tiles.h, inside a translation unit compiled with -ffp-contract=off.
#pragma once
#include "rt_tiles.h"

// rt_wave_common.h lets the compiler fuse the BOUNDS it defines; what follows is the reference's arithmetic again
#pragma clang fp contract(off)

namespace uobrt {
namespace {

constexpr int kShadeWaves = 4;              // waves per workgroup (independent after the table is staged)
// Work counters of a shade call (rt_debug_shade_stats)
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

// The table into the workgroup's LDS (kJumpWords words); the caller's barrier follows
__device__ __forceinline__ void stage_shade_jump(uint32_t* jump, int tid, int nthreads) {
  for (int i = tid; i < kJumpWords; i += nthreads) jump[i] = reinterpret_cast<const uint32_t*>(&kShadeJump)[i];
}

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

// One persistent wave: pulls runs of `run` groups of whole points from the queue head (the first word of `queue`) until the npoints points are taken.
// lane = (point, sample): with S < 64 a wave takes floor(64 / S) points (MULTI = false); with S >= 64 one point in
// ceil(S / 64) passes (MULTI = true).  P: fill_params with the call's light (+ use_tiled_scene when BOXES); tile = this
// wave's 4 * kQTile float4 of LDS, jump = the staged table.  Counters are added to: w (SH_* slots, wave-uniform), this
// LANE's triangle tests, and the rays outside the certificates' domain (wave-uniform).
template <bool BOXES, bool MULTI, class IO>
__device__ __forceinline__ void shade_groups(const FrameParams& P, const IO& io, long npoints, unsigned long long* queue, int run,
                                             float4* tile, const uint32_t* jump, int lane, unsigned long long (&w)[SH_SLOTS],
                                             unsigned long long& tests, unsigned long long& unculled) {
  const int S = P.S;
  const int ppw = MULTI ? 1 : 64 / S;                         // whole points per wave
  const int smagic = (65536 + S - 1) / S;                     // lane / S == (lane * smagic) >> 16 for lane < 64 (FrameParams::aa_magic)
  const int passes = MULTI ? (S + 63) >> 6 : 1;               // 64-sample passes per point (MULTI: S >= 64, one point per wave)
  const long ngroups = (npoints + ppw - 1) / ppw;
  const f3 light = mk(P.light[0], P.light[1], P.light[2]);
  unsigned int* const head = reinterpret_cast<unsigned int*>(queue);
  Work wk;                                    // (the counting slot of shadow_spheres<false>: never written)
  for (;;) {
    const unsigned int g0 = queue_pop(head, lane);
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
      if (have) io.load(k, pt, gid);
      const LightSetup l = light_setup(light, pt);
      const bool skip = have && !io.trace_all() && l.term == 0.0f;    // the frame's term == 0 skip
      w[SH_POINTS] += __popcll(ballot(have && si == 0));
      w[SH_SKIPPED] += __popcll(ballot(skip && si == 0));
      uint32_t r0 = rng_seed(gid, 0), r1 = rng_seed(gid, 1), r2 = rng_seed(gid, 2);     // the state after kernels.cl:319
      int unshadowed = 0;
      for (int pass = 0; pass < passes; ++pass) {
        const bool act = have && !skip && pass * 64 + si < S;
        if (ballot(act) == 0ull) break;                           // (every point of the group skipped)
        const f3 jit = mk(crush1(rng_advance(jump, r0, si + 1), P.spread), crush1(rng_advance(jump, r1, si + 1), P.spread),
                          crush1(rng_advance(jump, r2, si + 1), P.spread));
        const f3 d = l.dir + jit;
        TileHit h = no_hit();                                     // (the closest-hit slot of the shared walk: unused by SHADOW)
        bool blocked = false;
        w[SH_RAYS] += __popcll(ballot(act)); w[SH_WAVES] += 1;
        tile_walk<true, BOXES>(P, tile, lane, act, l.start, d, l.radius_sq, h, blocked, unculled, w[SH_BUNDLE_TILES],
                               w[SH_TESTED_TILES], tests);
        const bool lit = act && !blocked && !shadow_spheres<false>(P, l.start, d, l.radius_sq, wk);
        const int lb = opaque(lane);
        const int plb = MULTI ? 0 : (lb * smagic) >> 16;
        const unsigned long long seg = MULTI ? ~0ull : (((1ull << S) - 1ull) << (plb < ppw ? plb * S : 0));   // the point's lanes
        unshadowed += __popcll(ballot(lit) & seg);
        if (pass + 1 < passes) { r0 = rng_advance(jump, r0, 64); r1 = rng_advance(jump, r1, 64); r2 = rng_advance(jump, r2, 64); }
      }
      const int lc = opaque(lane);
      const int plc = MULTI ? 0 : (lc * smagic) >> 16;
      const long kc = g * ppw + plc;
      if (plc < ppw && kc < npoints && (MULTI ? lc : lc - plc * S) == 0) {      // the point's first lane
        float total = 0.0f;
        if (unshadowed < S) total += 0.0f * l.term;               // a blocked sample adds 0*term (NaN/inf-faithful)
#pragma unroll 4
        for (int i = 0; i < unshadowed; ++i) total += l.term;
        io.store(kc, div_count(total, S, P.inv_S), unshadowed);
      }
    }
  }
}

// Groups per hand-out, up to 32: a wave gets about 16 hand-outs without a tiled copy, where the groups cost much the same,
// and about 64 on a mesh, where a group on the mesh costs many times a group on a wall (measured on the 100 026-triangle
// scene, 2^18 points: runs of 3 took 59.8 ms, single groups 51.9)
__host__ __device__ inline int shade_run(long ngroups, long waves, bool tiled) {
  const long per = ngroups / (waves * (tiled ? 64 : 16));
  return (int)(per < 1 ? 1 : per > 32 ? 32 : per);
}

}  // namespace
}  // namespace uobrt
