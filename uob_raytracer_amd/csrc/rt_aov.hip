// rt_aov.hip — the AOV pass (rt_render_aov / rt_render_aov_device, include/uob_rt.h): what every pixel of a view SEES —
// primitive id, depth, position, normal, albedo and the primary ray's direction — i.e. the frame's primary pass without the
// shading.  Every plane carries the bits of the brute-force closest hit (single_ray_intersections, kernels.cl:168-241) of
// the frame's own primary ray (primary_ray, rt_trace.h) — DESIGN.md 4.6.
//
// Lanes: `sample` >= 0: a wave = an 8x8-pixel block, lane (l & 7, l >> 3), one sample per pixel; RT_AOV_ALL_SAMPLES: a wave =
// 64 consecutive (pixel, sample) elements of one pixel row.  Either way element e of a plane belongs to lane e of a run, so
// a float4 plane is stored 16 B per lane, 128 B (a block's row) or 1 KB (a run) contiguous.
// Contexts without a tiled copy (n <= 64, RT_FLAG_GENERIC_KERNEL): rt_aov_flat, the scene staged in LDS once per workgroup
// with the camera-dependent terms of the primary-ray test (stage_triangles), closest_hit_primary per lane.
// Tiled contexts (n > 64): rt_aov_tiled, persistent waves pulling runs of four jobs (queue_pop), each job through the walk
// every call beside the frame shares, tile_walk<false> (rt_tiles.h), with ONE step of its own:
//   1. the candidate tiles of the wave are those of the screen cells its pixels lie in (ScreenCellCandidates below, the
//      walk's candidate policy: the frame's own masks, rt_bin_primary run for this view in front of the kernel; no masks —
//      RT_FLAG_NO_TILE_BINS, up to 16 tiles — = every tile);
//   2. - 3. the walk's: the tile certificate per lane, the tile's records built into the wave's LDS, lane = triangle bounding
//      the wave's bundle (task_bound), the reference's test on the survivors with the original-order tie rule (closer);
//   4. the hit finished from the tiled arrays (finish_hit), then the spheres.
// Every skip is one of those certificates ("the reference's test cannot accept"), so skipping changes no bit.
// A plane that was not asked for (nullptr) costs a wave-uniform branch.
// Compiled with -ffp-contract=off: see rt_math.h for the numerics contract.
#include "rt_host.h"
#include "rt_tiles.h"

// rt_wave_common.h lets the compiler fuse the BOUNDS it defines; what follows is the reference's arithmetic again
#pragma clang fp contract(off)

namespace uobrt {

namespace {

constexpr int kAovWaves = 4;                // waves per workgroup (independent: no barriers between them)
constexpr int kAovRun = 4;                  // consecutive jobs per hand-out of the tiled kernel's queue
// Work counters of a pass (rt_debug_aov_stats), then the tiled kernel's queue head
enum { A_SAMPLES, A_WAVES, A_TILES, A_MASK_TILES, A_TESTED_TILES, A_TRI_TESTS, A_SLOTS = 8 };

// This lane's element of job `job`: pixel column, packed local row, AA sample (dy * aa_x + dx), element index in the planes.
// per_row = 8x8 blocks per block row (one sample) / 64-element runs per pixel row (ALL)
struct AovLane {
  int x, lr, a;
  bool valid;
  size_t e;
};
template <bool ALL>
__device__ __forceinline__ AovLane aov_lane(const FrameParams& P, int job, int per_row, int lane, int sample) {
  AovLane L;
  const int jr = job / per_row, jc = job - jr * per_row;
  if (ALL) {
    const int aa = P.aa_x * P.aa_y;
    const int idx = jc * 64 + lane;
    L.x = idx / aa; L.a = idx - L.x * aa; L.lr = jr;
    L.e = (size_t)jr * P.W * aa + idx;
  } else {
    L.x = jc * 8 + (lane & 7); L.lr = jr * 8 + (lane >> 3); L.a = sample;
    L.e = (size_t)L.lr * P.W + L.x;
  }
  L.valid = L.x < P.W && L.lr < P.owned_rows;
  return L;
}

// The frame's primary ray of the element (a lane past the frame gets the ray of the nearest pixel inside: never stored)
__device__ __forceinline__ Ray aov_ray(const FrameParams& P, const AovLane& L, int& y) {
  const int x = L.x < P.W ? L.x : P.W - 1;
  y = band_global_row(P, L.lr < P.owned_rows ? L.lr : P.owned_rows - 1);
  const int ay = L.a / P.aa_x;
  return primary_ray(P, x, y, L.a - ay * P.aa_x, ay);
}

__device__ __forceinline__ void store_planes(const AovPlanes& A, size_t e, const Ray& ray) {
  const bool hit = ray.tri != -1;
  // (component-wise selects: a select between two float4 objects is lowered through a stack slot)
  auto sel = [&](float x, float y, float z, float w) { return make_float4(hit ? x : 0.f, hit ? y : 0.f, hit ? z : 0.f, hit ? w : 0.f); };
  if (A.direction) A.direction[e] = make_float4(ray.dir.x, ray.dir.y, ray.dir.z, 0.f);
  if (A.prim) A.prim[e] = ray.tri;
  if (A.position) A.position[e] = sel(ray.P.x, ray.P.y, ray.P.z, 1.0f);
  if (A.normal) A.normal[e] = sel(ray.N.x, ray.N.y, ray.N.z, 0.f);
  if (A.albedo) A.albedo[e] = sel(ray.col.x, ray.col.y, ray.col.z, ray.col.w);
  if (A.depth) {
    const f3 d = ray.P - ray.start;
    A.depth[e] = hit ? sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z) : __builtin_inff();
  }
}

// tile_walk's candidate tiles for the AOV pass: those of the screen cells that the wave's pixels lie in (masks = the view's
// screen-cell masks, `words` 64-bit words per cell; nullptr = every tile).  cell = this lane's screen cell, active = the
// lanes that have an element: a wave's pixels lie in one to three cells (a band edge, a run across a cell edge).
struct ScreenCellCandidates {
  const unsigned long long* __restrict__ masks;
  int words, cell;
  unsigned long long active;
  template <class CLEAR>
  __device__ __forceinline__ unsigned long long operator()(int base, int, int ntiles, const CLEAR&) const {
    unsigned long long cand = ~0ull;
    if (masks) {
      cand = 0ull;
      for (unsigned long long rem = active; rem != 0ull;) {
        const int cid = __builtin_amdgcn_readlane(cell, __builtin_ctzll(rem));
        rem &= ~ballot(cell == cid);
        cand |= masks[(size_t)cid * words + (base >> 6)];
      }
    }
    if (ntiles - base < 64) cand &= (1ull << (ntiles - base)) - 1ull;   // (the tail of the last word)
    return cand;
  }
};

}  // namespace

// Contexts without a tiled copy: one lane per element over the whole scene in original order, the scene in LDS unless BIG
// (then P.records holds this view's staged records)
template <bool ALL, bool BIG>
__global__ __launch_bounds__(64 * kAovWaves) void rt_aov_flat(const FrameParams P, const AovPlanes A, int sample, int njobs, int per_row,
                                                               unsigned long long* __restrict__ stats) {
  extern __shared__ float4 lds_dyn[];
  const float4* lds = BIG ? P.records : lds_dyn;
  if (!BIG) {
    stage_triangles(P, lds_dyn, threadIdx.x, 64 * kAovWaves);
    __syncthreads();
  }
  const LdsScene S = lds_scene(lds, P.n);
  const int lane = threadIdx.x & 63;
  Work wk;
  unsigned long long w[A_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tests = 0;
  for (int job = blockIdx.x * kAovWaves + (threadIdx.x >> 6); job < njobs; job += gridDim.x * kAovWaves) {
    const AovLane L = aov_lane<ALL>(P, job, per_row, lane, sample);
    w[A_SAMPLES] += __popcll(ballot(L.valid)); w[A_WAVES] += 1;
    if (!L.valid) continue;
    int y;
    Ray ray = aov_ray(P, L, y);
    closest_hit_primary<false>(S, P, ray, wk);
    tests += (unsigned long long)P.n;
    store_planes(A, L.e, ray);
  }
  flush_counters(stats, w, A_TRI_TESTS, tests);
}

// Tiled contexts (P = the tiled copy: verts / normals / colors / orig / tile_box of use_tiled_scene; P.screen_masks = this
// view's candidate-tile masks or nullptr).  See the top of the file for the steps.
// (amdgpu_waves_per_eu(5), as rt_query_tiled: with the walk in the shared function the one-sample instantiation is allocated
// 98 vector registers instead of 92, i.e. 4 waves per SIMD instead of 5; held to 5 it stays within 96 without spills)
template <bool ALL>
__global__ __launch_bounds__(64 * kAovWaves) __attribute__((amdgpu_waves_per_eu(5)))
void rt_aov_tiled(const FrameParams P, const AovPlanes A, int sample, int njobs, int per_row, unsigned long long* __restrict__ stats) {
  __shared__ float4 s_tile[kAovWaves][4 * kQTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nwords = ((P.n + kQTile - 1) / kQTile + 63) >> 6;
  const int nruns = (njobs + kAovRun - 1) / kAovRun;
  unsigned int* const head = reinterpret_cast<unsigned int*>(stats + A_SLOTS);
  unsigned long long w[A_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tests = 0;
  unsigned long long unculled = 0;            // (tile_walk counts the rays outside the domain; an AOV pass does not report them)
  Work wk;
  for (;;) {
    const unsigned int g = queue_pop(head, lane);
    if (g >= (unsigned int)nruns) break;
    for (int job = (int)g * kAovRun; job < ((int)g + 1) * kAovRun && job < njobs; ++job) {
      const AovLane L = aov_lane<ALL>(P, job, per_row, lane, sample);
      const bool act = L.valid;
      int y;
      Ray ray = aov_ray(P, L, y);
      w[A_SAMPLES] += __popcll(ballot(act)); w[A_WAVES] += 1;
      const int cell = (y >> kScreenCellLog) * P.scx + ((L.x < P.W ? L.x : P.W - 1) >> kScreenCellLog);
      const ScreenCellCandidates cells{P.screen_masks, nwords, cell, ballot(act)};
      TileHit h = no_hit();
      bool blocked = false;                   // (the any-hit slot of the shared walk: unused by closest hit)
      tile_walk<false>(P, s_tile[wave], lane, act, ray.start, ray.dir, 0.0f, h, blocked, unculled, w[A_MASK_TILES], w[A_TESTED_TILES],
                       tests, cells);
      if (act) {
        finish_hit(P, h, ray);
        float current_t = h.t;
        closest_spheres<false>(P, ray, current_t, wk);
        store_planes(A, L.e, ray);
      }
    }
  }
  flush_counters(stats, w, A_TRI_TESTS, tests);
}

template __global__ void rt_aov_flat<false, false>(const FrameParams, const AovPlanes, int, int, int, unsigned long long*);
template __global__ void rt_aov_flat<false, true>(const FrameParams, const AovPlanes, int, int, int, unsigned long long*);
template __global__ void rt_aov_flat<true, false>(const FrameParams, const AovPlanes, int, int, int, unsigned long long*);
template __global__ void rt_aov_flat<true, true>(const FrameParams, const AovPlanes, int, int, int, unsigned long long*);
template __global__ void rt_aov_tiled<false>(const FrameParams, const AovPlanes, int, int, int, unsigned long long*);
template __global__ void rt_aov_tiled<true>(const FrameParams, const AovPlanes, int, int, int, unsigned long long*);

int aov_stats_words() { return A_SLOTS + 1; }

// P: fill_params of the view (+ use_tiled_scene when tiled; P.screen_masks = the view's masks, already built, or nullptr);
// without a tiled copy and beyond one LDS stage, P.records must already hold the view's staged records.
// sample < 0 = every AA sample.  stats: aov_stats_words() zeroed 64-bit words.
void launch_aov(const FrameParams& P, bool tiled, const AovPlanes& A, int sample, unsigned long long* stats, int cus, hipStream_t stream) {
  typedef void (*Kernel)(const FrameParams, const AovPlanes, int, int, int, unsigned long long*);
  const int aa = P.aa_x * P.aa_y;
  const bool all = sample < 0 && aa > 1;
  const int per_row = all ? (int)(((long)P.W * aa + 63) / 64) : (P.W + 7) / 8;
  const int njobs = per_row * (all ? P.owned_rows : (P.owned_rows + 7) / 8);   // <= 2^26: a frame has at most 2^24 pixels, 256 samples each
  const int s = sample < 0 ? 0 : sample;
  const dim3 block(64 * kAovWaves);
  if (tiled) {
    // (the persistent grid: the resident workgroups of whichever instantiation holds fewer, so a view's passes run on grids
    // of one size per job count)
    const int per_cu = std::min(blocks_per_cu(reinterpret_cast<const void*>(&rt_aov_tiled<false>), 64 * kAovWaves),
                                blocks_per_cu(reinterpret_cast<const void*>(&rt_aov_tiled<true>), 64 * kAovWaves));
    const Kernel kernel = all ? &rt_aov_tiled<true> : &rt_aov_tiled<false>;
    const dim3 grid(grid_blocks(((njobs + kAovRun - 1) / kAovRun + kAovWaves - 1) / kAovWaves, (long)cus * per_cu));
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, P, A, s, njobs, per_row, stats);
    return;
  }
  const bool big = P.n > kLdsMaxTriangles;
  const Kernel kernel = all ? (big ? &rt_aov_flat<true, true> : &rt_aov_flat<true, false>)
                            : (big ? &rt_aov_flat<false, true> : &rt_aov_flat<false, false>);
  const size_t lds = big ? 0 : (size_t)P.n * kLdsRecords * sizeof(float4);
  hipLaunchKernelGGL(kernel, dim3(grid_blocks((njobs + kAovWaves - 1) / kAovWaves, (long)cus * 8)), block, lds, stream, P, A, s, njobs, per_row, stats);
}

}  // namespace uobrt
