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
// Tiled contexts (n > 64): rt_aov_tiled, persistent waves pulling runs of four jobs:
//   1. the candidate tiles of the wave are those of the screen cells its pixels lie in (the frame's own masks, rt_bin_primary
//      run for this view in front of the kernel; no masks — RT_FLAG_NO_TILE_BINS, up to 16 tiles — = every tile);
//   2. - 4. exactly steps 2 - 4 of rt_query_tiled (rt_ray_query.hip): the tile certificate per lane, the tile's records built
//      into the wave's LDS, lane = triangle bounding the wave's bundle (task_bound), the reference's test on the survivors with
//      the original-order tie rule (closer), the hit finished from the tiled arrays, then the spheres.
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
constexpr int kATile = 64;                  // triangles per tile of the tiled copy (rt_kernel_mesh.hip kTile)
constexpr int kAovRun = 4;                  // consecutive jobs per hand-out of the tiled kernel's queue
// Work counters of a pass (rt_debug_aov_stats), then the tiled kernel's queue head
enum { A_SAMPLES, A_WAVES, A_TILES, A_MASK_TILES, A_TESTED_TILES, A_TRI_TESTS, A_SLOTS = 8 };

// One atomic add per counter and wave, at its exit (all lanes active)
__device__ __forceinline__ void flush_aov_stats(unsigned long long* stats, const unsigned long long (&w)[A_SLOTS], unsigned long long lane_tests) {
  const unsigned long long tests = wave_sum(lane_tests);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < A_SLOTS; ++q) {
      const unsigned long long v = q == A_TRI_TESTS ? tests : w[q];
      if (v) atomicAdd(&stats[q], v);
    }
  }
}

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
  flush_aov_stats(stats, w, tests);
}

// Tiled contexts (P = the tiled copy: verts / normals / colors / orig / tile_box of use_tiled_scene; P.screen_masks = this
// view's candidate-tile masks or nullptr).  See the top of the file for the steps.
template <bool ALL>
__global__ __launch_bounds__(64 * kAovWaves) void rt_aov_tiled(const FrameParams P, const AovPlanes A, int sample, int njobs, int per_row,
                                                                unsigned long long* __restrict__ stats) {
  __shared__ float4 s_tile[kAovWaves][4 * kATile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4* const tv0 = s_tile[wave];             // v0 | material
  float4* const te1 = tv0 + kATile;             // e1 | original index
  float4* const te2 = tv0 + 2 * kATile;         // e2
  float4* const tc = tv0 + 3 * kATile;          // cof(e1, e2)
  const int n = P.n, ntiles = (n + kATile - 1) / kATile, nwords = (ntiles + 63) >> 6;
  const int nruns = (njobs + kAovRun - 1) / kAovRun;
  unsigned int* const head = reinterpret_cast<unsigned int*>(stats + A_SLOTS);
  const bool bins = P.screen_masks != nullptr;
  unsigned long long w[A_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tests = 0;
  Work wk;
  for (;;) {
    unsigned int g = 0u;
    if (lane == 0) g = atomicAdd(head, 1u);
    g = (unsigned int)__builtin_amdgcn_readfirstlane((int)g);
    if (g >= (unsigned int)nruns) break;
    for (int job = (int)g * kAovRun; job < ((int)g + 1) * kAovRun && job < njobs; ++job) {
      const AovLane L = aov_lane<ALL>(P, job, per_row, lane, sample);
      const bool act = L.valid;
      int y;
      Ray ray = aov_ray(P, L, y);
      const f3 o = ray.start, d = ray.dir;
      const bool indom = act && in_query_domain(o, d);
      const bool brute = act && !indom;             // every triangle of every candidate tile
      const unsigned long long brm = ballot(brute);
      w[A_SAMPLES] += __popcll(ballot(act)); w[A_WAVES] += 1;
      // the wave's bundle (only while no lane is outside the domain)
      const BounceBundle bnd = bounce_bundle(indom, o, d);
      const bool bundle_ok = brm == 0ull && bnd.mode == 1;
      const float dl = 1.0001f * bsqrt(dot3(d, d)) * 1.0001f;                               // >= |d|_2 of this lane's ray
      const f3 nd = -d;
      // screen cell of this lane's pixel: a wave's pixels lie in one to three of them (a band edge, a run across a cell edge)
      const int cell = (y >> kScreenCellLog) * P.scx + ((L.x < P.W ? L.x : P.W - 1) >> kScreenCellLog);
      TileHit h = no_hit();
      for (int wi = 0; wi < nwords; ++wi) {
        unsigned long long cand = 0ull;
        if (bins) {
          for (unsigned long long rem = ballot(act); rem != 0ull;) {
            const int cid = __builtin_amdgcn_readlane(cell, __builtin_ctzll(rem));
            rem &= ~ballot(cell == cid);
            cand |= P.screen_masks[(size_t)cid * nwords + wi];
          }
        } else {
          cand = ~0ull;
        }
        if (wi == nwords - 1 && (ntiles & 63)) cand &= (1ull << (ntiles & 63)) - 1ull;
        w[A_MASK_TILES] += __popcll(cand);
        for (unsigned long long m = uniform64(cand); m != 0ull; m &= m - 1ull) {
          const int tt = wi * 64 + __builtin_ctzll(m);
          bool mine = act;
          if (mine && !brute) mine = !tile_clear_for_bundle(P.tile_box + (size_t)3 * tt, o, d, 0.0f, 0.0f, dl);
          if (ballot(mine) == 0ull) continue;
          wave_lds_sync();                          // the previous tile's records are no longer read
          {
            const int gi = tt * kATile + lane;
            if (gi < n) {
              const f3 v0 = xyz(P.verts[3 * gi]), e1 = xyz(P.verts[3 * gi + 1]) - v0, e2 = xyz(P.verts[3 * gi + 2]) - v0;
              const f3 cf = cof(e1, e2);
              tv0[lane] = make_float4(v0.x, v0.y, v0.z, P.colors[gi].w);
              te1[lane] = make_float4(e1.x, e1.y, e1.z, __int_as_float(P.orig[gi]));
              te2[lane] = make_float4(e2.x, e2.y, e2.z, 0.f);
              tc[lane] = make_float4(cf.x, cf.y, cf.z, 0.f);
            } else {
              tv0[lane] = make_float4(0.f, 0.f, 0.f, -1.0f);
              te1[lane] = te2[lane] = tc[lane] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
          }
          wave_lds_sync();
          const int nc = (n - tt * kATile) < kATile ? (n - tt * kATile) : kATile;
          unsigned long long K = nc == 64 ? ~0ull : ((1ull << nc) - 1ull);
          if (bundle_ok)
            K &= ~ballot(task_bound(tri_lane(tv0, te1, te2, tc, lane), bnd.s0, bnd.D0, bnd.es, bnd.ed, 2e-6f * bnd.dl, 0.0f, bnd.dl).clear);
          if (K == 0ull) continue;
          w[A_TESTED_TILES] += 1;
          if (mine) {
            // (uniform64: a loop inside a divergent `if` otherwise keeps its wave-uniform mask in vector registers)
            for (unsigned long long mm = uniform64(K); mm != 0ull; mm &= mm - 1ull) {
              const int i = __builtin_ctzll(mm);
              ++tests;
              const float4 e14 = te1[i];
              const f3 v0 = xyz(tv0[i]), e1 = xyz(e14), e2 = xyz(te2[i]), c = xyz(tc[i]);
              const f3 b = o - v0;                                        // kernels.cl:176-206
              const float detA_recip = rcp_exact(detc(nd, c));
              const float tq = detc(b, c) * detA_recip;
              const float u = detc(nd, cof(b, e2)) * detA_recip;
              const float v = detc(nd, cof(e1, b)) * detA_recip;
              const int oi = __float_as_int(e14.w);
              if (u >= 0 && v >= 0 && (u + v) <= 1 && tq >= 0 && closer(tq, oi, h)) h = TileHit{tq, u, v, tt * kATile + i, oi};
            }
          }
        }
      }
      if (act) {
        if (h.best >= 0) {                          // set_hit (kernels.cl:198-201) on the tiled arrays
          const int j = h.best;
          const f3 v0 = xyz(P.verts[3 * j]), e1 = xyz(P.verts[3 * j + 1]) - v0, e2 = xyz(P.verts[3 * j + 2]) - v0;
          ray.tri = h.orig;
          ray.P = (v0 + h.u * e1) + h.v * e2;
          ray.N = xyz(P.normals[j]);
          ray.col = P.colors[j];
        }
        float current_t = h.t;
        closest_spheres<false>(P, ray, current_t, wk);
        store_planes(A, L.e, ray);
      }
    }
  }
  flush_aov_stats(stats, w, tests);
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
  const int aa = P.aa_x * P.aa_y;
  const bool all = sample < 0 && aa > 1;
  const int per_row = all ? (int)(((long)P.W * aa + 63) / 64) : (P.W + 7) / 8;
  const int njobs = per_row * (all ? P.owned_rows : (P.owned_rows + 7) / 8);   // <= 2^26: a frame has at most 2^24 pixels, 256 samples each
  const int s = sample < 0 ? 0 : sample;
  const dim3 block(64 * kAovWaves);
  if (tiled) {
    static int per_cu = 0;                      // resident workgroups per CU (the persistent grid)
    if (per_cu == 0) {
      int a = 0, b = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, reinterpret_cast<const void*>(&rt_aov_tiled<false>), 64 * kAovWaves, 0) != hipSuccess) a = 2;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, reinterpret_cast<const void*>(&rt_aov_tiled<true>), 64 * kAovWaves, 0) != hipSuccess) b = 2;
      per_cu = std::max(1, std::min(a, b));
    }
    const long want = ((njobs + kAovRun - 1) / kAovRun + kAovWaves - 1) / kAovWaves;
    const long full = (long)cus * per_cu;
    const dim3 grid((unsigned)(want < full ? (want > 0 ? want : 1) : full));
    if (all) hipLaunchKernelGGL((rt_aov_tiled<true>), grid, block, 0, stream, P, A, s, njobs, per_row, stats);
    else hipLaunchKernelGGL((rt_aov_tiled<false>), grid, block, 0, stream, P, A, s, njobs, per_row, stats);
    return;
  }
  const long blocks = (njobs + kAovWaves - 1) / kAovWaves;
  const long full = (long)cus * 8;
  const dim3 grid((unsigned)(blocks < full ? (blocks > 0 ? blocks : 1) : full));
  const bool big = P.n > kLdsMaxTriangles;
  const size_t lds = big ? 0 : (size_t)P.n * kLdsRecords * sizeof(float4);
  if (all) {
    if (big) hipLaunchKernelGGL((rt_aov_flat<true, true>), grid, block, 0, stream, P, A, s, njobs, per_row, stats);
    else hipLaunchKernelGGL((rt_aov_flat<true, false>), grid, block, lds, stream, P, A, s, njobs, per_row, stats);
  } else {
    if (big) hipLaunchKernelGGL((rt_aov_flat<false, true>), grid, block, 0, stream, P, A, s, njobs, per_row, stats);
    else hipLaunchKernelGGL((rt_aov_flat<false, false>), grid, block, lds, stream, P, A, s, njobs, per_row, stats);
  }
}

}  // namespace uobrt
