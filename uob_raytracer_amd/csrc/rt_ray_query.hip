// rt_ray_query.hip — ray queries on a context's scene (rt_trace_rays / rt_trace_rays_device, include/uob_rt.h): the
// closest hit (single_ray_intersections, kernels.cl:168-241) or the shadow test (in_shadow, :243-311) of caller rays,
// bit-identical to the brute-force diagnostic rt_debug_trace_rays (rt_kernel_generic.hip rt_trace_rays).
//
// Contexts without a tiled copy (n <= 64, RT_FLAG_GENERIC_KERNEL): rt_query_flat, one lane per ray over the whole scene
// in original order, the scene staged in LDS once per workgroup (or, beyond one LDS stage, the query's own records).
// Tiled contexts (n > 64): rt_query_tiled, persistent waves, 64 consecutive rays per wave:
//   1. lane = tile, 64 tiles per pass: the wave's rays bounded as one bundle (bounce_bundle) against each tile's box,
//      normal cone and sliver measure (tile_clear_for_bundle, rt_tiles.h) -> the candidate tiles of the pass;
//   2. per candidate tile, the same certificate for each lane's own ray (es = ed = 0), ballot: no lane -> next tile;
//   3. the tile's records v0|material, e1|original index, e2, c = cof(e1, e2) are built into the wave's LDS from the tiled
//      copy, lane = triangle bounds the bundle (task_bound; on curved meshes the tiles' normal cones are wide, and this is
//      where most of the work goes away) and lane = ray tests the survivors with the reference's
//      arithmetic: closest hit carried across tiles with the original-order tie rule (closer), shadow any-hit with an
//      early exit per lane and per wave;
//   4. the hit is finished from the tiled arrays (set_hit arithmetic), then the spheres (closest_spheres / shadow_spheres).
// Every skip is a certificate that the reference's test cannot accept, so skipping changes no bit.  The certificates are
// verified for |start| <= 2^16 and 2^-20 <= max |direction component| <= 2^16 (finite); a ray outside that domain
// needs every tile and every triangle, i.e. it gets the brute-force answer by construction.
// Compiled with -ffp-contract=off: see rt_math.h for the numerics contract.
#include "rt_tiles.h"

// rt_wave_common.h lets the compiler fuse the BOUNDS it defines; what follows is the reference's arithmetic again
#pragma clang fp contract(off)

namespace uobrt {

namespace {

constexpr int kQueryWaves = 4;              // waves per workgroup of rt_query_tiled (independent: no barriers between them)
constexpr int kQTile = 64;                  // triangles per tile of the tiled copy (rt_kernel_mesh.hip kTile)
// Work counters of a query (rt_debug_trace_stats), then the tiled kernel's queue head
enum { Q_RAYS, Q_WAVES, Q_TILES, Q_BUNDLE_TILES, Q_TESTED_TILES, Q_TRI_TESTS, Q_UNCULLED, Q_SLOTS = 8 };

// One atomic add per counter and wave, at its exit (all lanes active)
__device__ __forceinline__ void flush_stats(unsigned long long* stats, const unsigned long long (&w)[Q_SLOTS], unsigned long long lane_tests) {
  const unsigned long long tests = wave_sum(lane_tests);
  if ((threadIdx.x & 63) == 0) {
    for (int q = 0; q < Q_SLOTS; ++q) {
      const unsigned long long v = q == Q_TRI_TESTS ? tests : w[q];
      if (v) atomicAdd(&stats[q], v);
    }
  }
}

__device__ __forceinline__ void store_hit(float* out10, long k, const Ray& ray) {
  float* o = out10 + 10 * k;
  const bool hit = ray.tri != -1;
  o[0] = hit ? ray.P.x : 0.f; o[1] = hit ? ray.P.y : 0.f; o[2] = hit ? ray.P.z : 0.f;
  o[3] = hit ? ray.N.x : 0.f; o[4] = hit ? ray.N.y : 0.f; o[5] = hit ? ray.N.z : 0.f;
  o[6] = hit ? ray.col.x : 0.f; o[7] = hit ? ray.col.y : 0.f; o[8] = hit ? ray.col.z : 0.f; o[9] = hit ? ray.col.w : 0.f;
}

__device__ __forceinline__ Ray query_ray(f3 start, f3 dir) {
  Ray ray;
  ray.start = start; ray.dir = dir; ray.tri = -1; ray.medium = RT_AIR;
  ray.col = make_float4(0.f, 0.f, 0.f, 1.0f);
  ray.P = mk(0.f, 0.f, 0.f); ray.N = mk(0.f, 0.f, 0.f);
  return ray;
}

}  // namespace

// Contexts without a tiled copy: rt_trace_rays's mapping (one lane per ray, grid-stride), the scene in LDS unless BIG.
// SHADOW: in_shadow -> out_tri 0 / 1; else the closest hit -> out_tri, out10 (nullable; zeros on a miss).
template <bool SHADOW, bool BIG>
__global__ __launch_bounds__(256) void rt_query_flat(const FrameParams P, const float* __restrict__ rays, const float* __restrict__ r2,
                                                     long nray, int* __restrict__ out_tri, float* __restrict__ out10,
                                                     unsigned long long* __restrict__ stats) {
  extern __shared__ float4 lds_dyn[];
  const float4* lds = BIG ? P.records : lds_dyn;
  if (!BIG) {
    stage_triangles(P, lds_dyn, threadIdx.x, 256);
    __syncthreads();
  }
  const LdsScene S = lds_scene(lds, P.n);
  Work wk;
  for (int q = 0; q < 8; ++q) wk.v[q] = 0;
  unsigned long long w[Q_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (long base = (long)blockIdx.x * 256 + (threadIdx.x & ~63); base < nray; base += (long)gridDim.x * 256) {
    const long k = base + (threadIdx.x & 63);
    const unsigned long long am = ballot(k < nray);
    w[Q_RAYS] += __popcll(am); w[Q_WAVES] += 1; w[Q_UNCULLED] += __popcll(am);
    if (k >= nray) continue;
    const f3 start = mk(rays[6 * k], rays[6 * k + 1], rays[6 * k + 2]), dir = mk(rays[6 * k + 3], rays[6 * k + 4], rays[6 * k + 5]);
    if (SHADOW) {
      out_tri[k] = in_shadow<true>(S, P, start, dir, r2[k], wk) ? 1 : 0;
    } else {
      Ray ray = query_ray(start, dir);
      closest_hit<false>(S, P, ray, wk);
      wk.v[W_STRI] += (unsigned long long)P.n;
      out_tri[k] = ray.tri;
      if (out10) store_hit(out10, k, ray);
    }
  }
  flush_stats(stats, w, wk.v[W_STRI]);
}

// Tiled contexts (P = the tiled copy: verts / normals / colors / orig / tile_box of use_tiled_scene).  Persistent waves pull
// 64-ray groups from the queue head behind the counters; see the top of the file for the four steps.
template <bool SHADOW>
__global__ __launch_bounds__(64 * kQueryWaves) void rt_query_tiled(const FrameParams P, const float* __restrict__ rays,
                                                                    const float* __restrict__ r2, long nray, int* __restrict__ out_tri,
                                                                    float* __restrict__ out10, unsigned long long* __restrict__ stats) {
  __shared__ float4 s_tile[kQueryWaves][4 * kQTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4* const tv0 = s_tile[wave];             // v0 | material
  float4* const te1 = tv0 + kQTile;             // e1 | original index
  float4* const te2 = tv0 + 2 * kQTile;         // e2
  float4* const tc = tv0 + 3 * kQTile;          // cof(e1, e2)
  const int n = P.n, ntiles = (n + kQTile - 1) / kQTile;
  const long ngroups = (nray + 63) >> 6;
  unsigned int* const head = reinterpret_cast<unsigned int*>(stats + Q_SLOTS);
  unsigned long long w[Q_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tests = 0;
  Work wk;
  for (;;) {
    unsigned int g = 0u;
    if (lane == 0) g = atomicAdd(head, 1u);
    g = (unsigned int)__builtin_amdgcn_readfirstlane((int)g);
    if ((long)g >= ngroups) break;
    const long k = (long)g * 64 + lane;
    const bool act = k < nray;
    f3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 0.f);
    float rsq = 0.0f;
    if (act) {
      o = mk(rays[6 * k], rays[6 * k + 1], rays[6 * k + 2]);
      d = mk(rays[6 * k + 3], rays[6 * k + 4], rays[6 * k + 5]);
      if (SHADOW) rsq = r2[k];
    }
    const bool indom = act && in_query_domain(o, d);
    const bool brute = act && !indom;             // every tile, every triangle
    const unsigned long long brm = ballot(brute);
    w[Q_RAYS] += __popcll(ballot(act)); w[Q_WAVES] += 1; w[Q_UNCULLED] += __popcll(brm);
    // the wave's bundle (only while no lane is outside the domain: such a lane needs every tile anyway)
    const BounceBundle bnd = bounce_bundle(indom, o, d);
    const bool bundle_ok = brm == 0ull && bnd.mode == 1;
    const float d2 = 1.0001f * bsqrt(wave_max_pos(indom ? dot3(d, d) : 0.0f)) * 1.0001f;   // >= |d|_2 of every ray of the bundle
    const float dl = 1.0001f * bsqrt(dot3(d, d)) * 1.0001f;                               // >= |d|_2 of this lane's ray
    const f3 nd = -d;
    TileHit h = no_hit();
    bool blocked = false;
    bool done = false;                            // SHADOW: every lane of the wave has found its blocker
    for (int base = 0; base < ntiles && !done; base += 64) {
      const int t = base + lane;
      bool need = t < ntiles;
      if (need && bundle_ok) need = !tile_clear_for_bundle(P.tile_box + (size_t)3 * t, bnd.s0, bnd.D0, bnd.es, bnd.ed, d2);
      const unsigned long long cand = ballot(need);
      w[Q_BUNDLE_TILES] += __popcll(cand);
      for (unsigned long long m = uniform64(cand); m != 0ull; m &= m - 1ull) {
        const int tt = base + __builtin_ctzll(m);
        bool mine = act && !(SHADOW && blocked);
        if (mine && !brute) mine = !tile_clear_for_bundle(P.tile_box + (size_t)3 * tt, o, d, 0.0f, 0.0f, dl);
        if (ballot(mine) == 0ull) continue;
        wave_lds_sync();                          // the previous tile's records are no longer read
        {
          const int gi = tt * kQTile + lane;
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
        const int nc = (n - tt * kQTile) < kQTile ? (n - tt * kQTile) : kQTile;
        unsigned long long K = nc == 64 ? ~0ull : ((1ull << nc) - 1ull);
        if (SHADOW) K &= ~ballot(tv0[lane].w == -1.0f);                 // glass casts no shadow (kernels.cl:250)
        if (bundle_ok)
          K &= ~ballot(task_bound(tri_lane(tv0, te1, te2, tc, lane), bnd.s0, bnd.D0, bnd.es, bnd.ed, 2e-6f * bnd.dl, 0.0f, bnd.dl).clear);
        if (K == 0ull) continue;
        w[Q_TESTED_TILES] += 1;
        if (mine) {
          // (uniform64: a loop inside a divergent `if` otherwise keeps its wave-uniform mask in vector registers)
          for (unsigned long long mm = uniform64(K); mm != 0ull; mm &= mm - 1ull) {
            const int i = __builtin_ctzll(mm);
            ++tests;
            const float4 e14 = te1[i];
            const f3 v0 = xyz(tv0[i]), e1 = xyz(e14), e2 = xyz(te2[i]), c = xyz(tc[i]);
            const f3 b = o - v0;
            const float detA_recip = rcp_exact(detc(nd, c));
            const float tq = detc(b, c) * detA_recip;
            if (SHADOW) {                                               // kernels.cl:258-274
              const f3 dv = tq * d;
              const float dist = dv.x * dv.x + dv.y * dv.y + dv.z * dv.z;
              if (tq >= 0 && dist < rsq) {
                const float u = detc(nd, cof(b, e2)) * detA_recip;
                const float v = detc(nd, cof(e1, b)) * detA_recip;
                if (u >= 0 && v >= 0 && (u + v) <= 1) { blocked = true; break; }
              }
            } else {                                                    // kernels.cl:176-206
              const float u = detc(nd, cof(b, e2)) * detA_recip;
              const float v = detc(nd, cof(e1, b)) * detA_recip;
              const int oi = __float_as_int(e14.w);
              if (u >= 0 && v >= 0 && (u + v) <= 1 && tq >= 0 && closer(tq, oi, h)) h = TileHit{tq, u, v, tt * kQTile + i, oi};
            }
          }
        }
        if (SHADOW && ballot(act && !blocked) == 0ull) { done = true; break; }
      }
    }
    if (act) {
      if (SHADOW) {
        out_tri[k] = (blocked || shadow_spheres<false>(P, o, d, rsq, wk)) ? 1 : 0;
      } else {
        Ray ray = query_ray(o, d);
        if (h.best >= 0) {                        // set_hit (kernels.cl:198-201) on the tiled arrays
          const int j = h.best;
          const f3 v0 = xyz(P.verts[3 * j]), e1 = xyz(P.verts[3 * j + 1]) - v0, e2 = xyz(P.verts[3 * j + 2]) - v0;
          ray.tri = h.orig;
          ray.P = (v0 + h.u * e1) + h.v * e2;
          ray.N = xyz(P.normals[j]);
          ray.col = P.colors[j];
        }
        float current_t = h.t;
        closest_spheres<false>(P, ray, current_t, wk);
        out_tri[k] = ray.tri;
        if (out10) store_hit(out10, k, ray);
      }
    }
  }
  flush_stats(stats, w, tests);
}

template __global__ void rt_query_flat<false, false>(const FrameParams, const float*, const float*, long, int*, float*, unsigned long long*);
template __global__ void rt_query_flat<false, true>(const FrameParams, const float*, const float*, long, int*, float*, unsigned long long*);
template __global__ void rt_query_flat<true, false>(const FrameParams, const float*, const float*, long, int*, float*, unsigned long long*);
template __global__ void rt_query_flat<true, true>(const FrameParams, const float*, const float*, long, int*, float*, unsigned long long*);
template __global__ void rt_query_tiled<false>(const FrameParams, const float*, const float*, long, int*, float*, unsigned long long*);
template __global__ void rt_query_tiled<true>(const FrameParams, const float*, const float*, long, int*, float*, unsigned long long*);

int query_stats_words() { return Q_SLOTS + 1; }

// P: fill_params of the context (+ use_tiled_scene when tiled); without a tiled copy and beyond one LDS stage, P.records
// must already hold the query's staged records.  stats: query_stats_words() zeroed 64-bit words.
void launch_query(const FrameParams& P, bool tiled, int what, const float* d_rays, const float* d_r2, long nray, int* d_tri,
                  float* d_out10, unsigned long long* stats, int cus, hipStream_t stream) {
  const bool shadow = what == RT_TRACE_IN_SHADOW;
  if (tiled) {
    static int per_cu = 0;                      // resident workgroups per CU (the persistent grid)
    if (per_cu == 0) {
      int a = 0, b = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, reinterpret_cast<const void*>(&rt_query_tiled<false>), 64 * kQueryWaves, 0) != hipSuccess) a = 2;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, reinterpret_cast<const void*>(&rt_query_tiled<true>), 64 * kQueryWaves, 0) != hipSuccess) b = 2;
      per_cu = std::max(1, std::min(a, b));
    }
    const long want = ((nray + 63) / 64 + kQueryWaves - 1) / kQueryWaves;
    const long full = (long)cus * per_cu;
    const dim3 grid((unsigned)(want < full ? want : full));
    if (shadow) hipLaunchKernelGGL((rt_query_tiled<true>), grid, dim3(64 * kQueryWaves), 0, stream, P, d_rays, d_r2, nray, d_tri, d_out10, stats);
    else hipLaunchKernelGGL((rt_query_tiled<false>), grid, dim3(64 * kQueryWaves), 0, stream, P, d_rays, d_r2, nray, d_tri, d_out10, stats);
    return;
  }
  const long blocks = (nray + 255) / 256;
  const dim3 grid((unsigned)(blocks < 4096 ? (blocks > 0 ? blocks : 1) : 4096));
  const bool big = P.n > kLdsMaxTriangles;
  const size_t lds = big ? 0 : (size_t)P.n * kLdsRecords * sizeof(float4);
  if (shadow) {
    if (big) hipLaunchKernelGGL((rt_query_flat<true, true>), grid, dim3(256), 0, stream, P, d_rays, d_r2, nray, d_tri, d_out10, stats);
    else hipLaunchKernelGGL((rt_query_flat<true, false>), grid, dim3(256), lds, stream, P, d_rays, d_r2, nray, d_tri, d_out10, stats);
  } else {
    if (big) hipLaunchKernelGGL((rt_query_flat<false, true>), grid, dim3(256), 0, stream, P, d_rays, d_r2, nray, d_tri, d_out10, stats);
    else hipLaunchKernelGGL((rt_query_flat<false, false>), grid, dim3(256), lds, stream, P, d_rays, d_r2, nray, d_tri, d_out10, stats);
  }
}

}  // namespace uobrt
