// rt_ray_query.hip — ray queries on a context's scene (rt_trace_rays / rt_trace_rays_device, include/uob_rt.h): the
// closest hit (single_ray_intersections, kernels.cl:168-241) or the shadow test (in_shadow, :243-311) of caller rays,
// bit-identical to the brute-force diagnostic rt_debug_trace_rays (rt_kernel_generic.hip rt_trace_rays).
//
// Contexts without a tiled copy (n <= 64, RT_FLAG_GENERIC_KERNEL): rt_query_flat, one lane per ray over the whole scene
// in original order, the scene staged in LDS once per workgroup (or, beyond one LDS stage, the query's own records).
// Tiled contexts (n > 64): rt_query_tiled, persistent waves, 64 consecutive rays per wave:
//   1.-3. tile_walk (rt_tiles.h, shared with rt_shade.hip, rt_radiance.hip and rt_aov.hip): the bundle bound per tile (the
//      walk's default candidate policy, BundleCandidates), the per-lane tile certificate, the
//      tile's records in the wave's LDS with lane = triangle bounding the bundle (task_bound; on curved meshes the tiles'
//      normal cones are wide, and this is where most of the work goes away) and lane = ray testing the survivors with the
//      reference's arithmetic: closest hit carried across tiles with the original-order tie rule (closer), shadow any-hit
//      with an early exit per lane and per wave;
//   4. the hit is finished from the tiled arrays (finish_hit: set_hit arithmetic), then the spheres (closest_spheres /
//      shadow_spheres).
// The queue pop (queue_pop) and the counter flush (flush_counters) are rt_tiles.h's too, as for every kernel beside the frame.
// Every skip is a certificate that the reference's test cannot accept, so skipping changes no bit.  The certificates are
// verified for |start| <= 2^16 and 2^-20 <= max |direction component| <= 2^16 (finite); a ray outside that domain
// needs every tile and every triangle, i.e. it gets the brute-force answer by construction.
// Compiled with -ffp-contract=off: see rt_math.h for the numerics contract.
#include "rt_host.h"
#include "rt_tiles.h"

// rt_wave_common.h lets the compiler fuse the BOUNDS it defines; what follows is the reference's arithmetic again
#pragma clang fp contract(off)

namespace uobrt {

namespace {

constexpr int kQueryWaves = 4;              // waves per workgroup of rt_query_tiled (independent: no barriers between them)
// Work counters of a query (rt_debug_trace_stats), then the tiled kernel's queue head
enum { Q_RAYS, Q_WAVES, Q_TILES, Q_BUNDLE_TILES, Q_TESTED_TILES, Q_TRI_TESTS, Q_UNCULLED, Q_SLOTS = 8 };

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
  flush_counters(stats, w, Q_TRI_TESTS, wk.v[W_STRI]);
}

// Tiled contexts (P = the tiled copy: verts / normals / colors / orig / tile_box of use_tiled_scene).  Persistent waves pull
// 64-ray groups from the queue head behind the counters; see the top of the file for the four steps.
// (amdgpu_waves_per_eu(5): with the walk in a shared function the closest-hit instantiation is allocated 102 vector registers
// instead of 93, i.e. 4 waves per SIMD instead of 5; held to 5 it takes 96, without spills)
template <bool SHADOW>
__global__ __launch_bounds__(64 * kQueryWaves) __attribute__((amdgpu_waves_per_eu(5)))
void rt_query_tiled(const FrameParams P, const float* __restrict__ rays, const float* __restrict__ r2, long nray,
                    int* __restrict__ out_tri, float* __restrict__ out10, unsigned long long* __restrict__ stats) {
  __shared__ float4 s_tile[kQueryWaves][4 * kQTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long ngroups = (nray + 63) >> 6;
  unsigned int* const head = reinterpret_cast<unsigned int*>(stats + Q_SLOTS);
  unsigned long long w[Q_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tests = 0;
  Work wk;
  for (;;) {
    const unsigned int g = queue_pop(head, lane);
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
    TileHit h = no_hit();
    bool blocked = false;
    w[Q_RAYS] += __popcll(ballot(act)); w[Q_WAVES] += 1;
    tile_walk<SHADOW>(P, s_tile[wave], lane, act, o, d, rsq, h, blocked, w[Q_UNCULLED], w[Q_BUNDLE_TILES], w[Q_TESTED_TILES], tests);
    if (act) {
      if (SHADOW) {
        out_tri[k] = (blocked || shadow_spheres<false>(P, o, d, rsq, wk)) ? 1 : 0;
      } else {
        Ray ray = query_ray(o, d);
        finish_hit(P, h, ray);
        float current_t = h.t;
        closest_spheres<false>(P, ray, current_t, wk);
        out_tri[k] = ray.tri;
        if (out10) store_hit(out10, k, ray);
      }
    }
  }
  flush_counters(stats, w, Q_TRI_TESTS, tests);
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
  typedef void (*Kernel)(const FrameParams, const float*, const float*, long, int*, float*, unsigned long long*);
  const bool shadow = what == RT_TRACE_IN_SHADOW;
  if (tiled) {
    // (the persistent grid: the resident workgroups of whichever instantiation holds fewer, so a context's closest-hit and
    // in-shadow queries run on grids of one size)
    const int per_cu = std::min(blocks_per_cu(reinterpret_cast<const void*>(&rt_query_tiled<false>), 64 * kQueryWaves),
                                blocks_per_cu(reinterpret_cast<const void*>(&rt_query_tiled<true>), 64 * kQueryWaves));
    const Kernel kernel = shadow ? &rt_query_tiled<true> : &rt_query_tiled<false>;
    const dim3 grid(grid_blocks(((nray + 63) / 64 + kQueryWaves - 1) / kQueryWaves, (long)cus * per_cu));
    hipLaunchKernelGGL(kernel, grid, dim3(64 * kQueryWaves), 0, stream, P, d_rays, d_r2, nray, d_tri, d_out10, stats);
    return;
  }
  const bool big = P.n > kLdsMaxTriangles;
  const Kernel kernel = shadow ? (big ? &rt_query_flat<true, true> : &rt_query_flat<true, false>)
                               : (big ? &rt_query_flat<false, true> : &rt_query_flat<false, false>);
  const size_t lds = big ? 0 : (size_t)P.n * kLdsRecords * sizeof(float4);
  hipLaunchKernelGGL(kernel, dim3(grid_blocks((nray + 255) / 256, 4096)), dim3(256), lds, stream, P, d_rays, d_r2, nray, d_tri, d_out10, stats);
}

}  // namespace uobrt
