// rt_tiles.h — what the kernels share of the tiled mesh copy (rt_scene.hip upload_tiled_scene).  The exact tile certificate and the
// closest-hit tie rule: the mesh kernel (rt_kernel_mesh.hip, bounce rays) and every kernel of the calls beside the frame.
// For those kernels — the ray queries (rt_ray_query.hip), rt_shade_points (rt_shade.hip, rt_shade_body.h), rt_radiance_rays
// (rt_radiance.hip) and the AOV pass (rt_aov.hip) — also the ONE tiled walk (tile_walk; where a pass's candidate tiles come
// from is a policy), the hit finisher (finish_hit), the pop of a persistent kernel's queue (queue_pop) and the flush of a
// wave's work counters (flush_counters).  Include after rt_wave_common.h.
#pragma once
#include "rt_wave_common.h"

namespace uobrt {
namespace {

// ---- bounce rays: may ANY ray of a bundle hit ANY triangle of a tile? -----------------------------------------------------
// The per-triangle bound (task_bound, lane = triangle) needs the tile in LDS; this one needs 48 bytes per tile and is asked
// lane = tile, 64 tiles per pass, before anything is loaded.  A plain ray-box test would NOT do: for a ray that lies in a
// triangle's plane all the determinants of the reference's test vanish, its t, u, v are rounding noise, and the reference may
// "hit" a triangle the ray passes at any distance — noise this library must reproduce.  The certificate:
//   With W1 = det(A1), W2 = det(A2), W0 = det(A) - W1 - W2 (the three edge functions; u = W1 / det(A), v = W2 / det(A),
//   1 - u - v = W0 / det(A)) and any n perpendicular to the ray's direction,   sum_i W_i n.(v_i - o) = 0   holds identically
//   (sum_i W_i (v_i - o) = det(A0) d).  Take n = d x e_k (k = x, y, z: the separating axes of a line and a box): if the
//   tile's box lies on one side of that plane through the ray, every a_i = n.(v_i - o) is in [gap, gap + 2 rad], gap > 0.
//   The reference accepts only if u >= 0, v >= 0, fl(u + v) <= 1, i.e. if the COMPUTED W_i all have det(A)'s sign (up to
//   4 eps of their magnitudes); by the identity that is possible only if all three computed W_i are within
//   Omega = 3 E (1 + 2 rad / gap) of zero, E <= 21 eps |d| (|b| + |e|) |e| bounding their rounding errors (eps = 2^-24).
//   And they are NOT all that small unless the ray lies in the triangle's plane:   max_i |W_i| >= 0.28 theta |c| |d|   where
//   theta <= max(|n_T . d| / |d|, |n_T . (o - v)| / bmax) (n_T the triangle's unit normal, bmax >= |o - v|): from
//   det(A) = sum W_i and, for in-plane g, sum W_i g.(v_i - o) = det(A0) g.d.  Per tile the normals lie in a cone (unit axis a,
//   chord chi = max |n_T -+ a|), so theta >= max(|a . d| / |d|, |a . (o - v)| / bmax) - chi, bounded over the bundle and the box.
//   Certified clear iff  gap > 0  and  theta >= 150 eps (4 + 6 rad / gap) (bmax + emax) eta   (factor of safety 2 included),
//   eta = max |e| / |e1 x e2| and emax = max |e| over the tile's triangles (rt_tile_sort.hip tile_data_host, uploaded by rt_scene.hip upload_tiled_scene).
// Bundle: origins s0 +- es, directions D0 +- ed per component, |d|_2 <= dmax2.  Conservative in every term; `false` = visit.
__device__ __forceinline__ bool tile_clear_for_bundle(const float4* __restrict__ tb, f3 s0, f3 D0, float es, float ed, float dmax2) {
  const float4 lo4 = tb[0], hi4 = tb[1], ax4 = tb[2];
  const float eta = lo4.w, emax = hi4.w, chi = ax4.w;
  const f3 axis = xyz(ax4);
  const f3 cB = 0.5f * (xyz(lo4) + xyz(hi4));
  // (half extents with the rounding of the staged e1 = v1 - v0, e2 = v2 - v0 and of cB itself)
  const float cs = 4e-7f * (norm_inf(xyz(lo4)) + norm_inf(xyz(hi4)));
  const f3 hB = mk(0.5f * (hi4.x - lo4.x) * 1.00001f + cs, 0.5f * (hi4.y - lo4.y) * 1.00001f + cs, 0.5f * (hi4.z - lo4.z) * 1.00001f + cs);
  const f3 r0 = cB - s0;
  const float esb = es * 1.0001f + 1e-6f * norm_inf(s0);
  const float bmax = 1.7321f * (norm_inf(r0) + fmaxf(fmaxf(hB.x, hB.y), hB.z) + esb);
  const float rr[3] = {r0.x, r0.y, r0.z}, dd[3] = {D0.x, D0.y, D0.z}, hh[3] = {hB.x, hB.y, hB.z};
  float ratio = 3.0e38f;                                               // smallest rad / gap over the axes that separate
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int j = (k + 1) % 3, l = (k + 2) % 3;
    const float t1 = dd[l] * rr[j], t2 = dd[j] * rr[l];
    const float f0 = t1 - t2;                                          // (d x e_k) . r up to sign
    const float dev = ed * (fabsf(rr[j]) + fabsf(rr[l])) + esb * (fabsf(dd[l]) + fabsf(dd[j])) + 2.0f * ed * esb;
    const float rad = hh[j] * (fabsf(dd[l]) + ed) + hh[l] * (fabsf(dd[j]) + ed);
    const float gap = fabsf(f0) - dev - rad - 1e-5f * (fabsf(t1) + fabsf(t2) + dev + rad);   // (minus this evaluation's own rounding)
    if (gap > 0.0f) ratio = fminf(ratio, rad / gap);
  }
  if (!(ratio < 1.0e30f)) return false;
  const float a1 = norm1(axis);
  const float k_line = (fabsf(bdot3(axis, D0)) - ed * a1) / dmax2;
  const float k_orig = (fabsf(bdot3(axis, r0)) - (fabsf(axis.x) * hB.x + fabsf(axis.y) * hB.y + fabsf(axis.z) * hB.z) - esb * a1) / bmax;
  const float theta = fmaxf(k_line, k_orig) * 0.9999f - chi;
  return theta >= 8.95e-6f * (4.0f + 6.0f * ratio) * (bmax + emax) * eta;     // 150 * 2^-24 = 8.94e-6
}

// A closest hit carried across tiles: t, barycentrics, position in the reordered mesh (-1: none yet), original index
struct TileHit { float t, u, v; int best, orig; };
__device__ __forceinline__ TileHit no_hit() { return TileHit{RT_MAXFLOAT, 0.f, 0.f, -1, 0x7fffffff}; }
// Does a hit at t on the triangle of original index `orig` replace h?  The reference visits the triangles in their ORIGINAL
// order and replaces the hit only for a strictly smaller t (kernels.cl:120): of equal t the lowest original index stays —
// whatever order the tiles come in.
__device__ __forceinline__ bool closer(float t, int orig, const TileHit& h) {
  return t < h.t || (t == h.t && h.best >= 0 && orig < h.orig);
}

// ---- shared by the kernels of the calls beside the frame: ray queries, shade, radiance, AOV ---------------------------------
// The domain over which the exact certificates hold: finite, |start| <= 2^16, 2^-20 <= max |direction component| <= 2^16
__device__ __forceinline__ bool in_query_domain(f3 o, f3 d) {
  const bool fin = fabsf(o.x) <= kMaxCoordinate && fabsf(o.y) <= kMaxCoordinate && fabsf(o.z) <= kMaxCoordinate &&
                   fabsf(d.x) <= kMaxCoordinate && fabsf(d.y) <= kMaxCoordinate && fabsf(d.z) <= kMaxCoordinate;   // (false for NaN)
  return fin && fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z)) >= 0x1p-20f;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// A persistent wave takes the next ticket of its kernel's queue: one returning atomic by lane 0, the ticket wave-uniform.
// What a ticket stands for (a group, a run of groups) and where the queue ends is the caller's.
__device__ __forceinline__ unsigned int queue_pop(unsigned int* head, int lane) {
  unsigned int g = 0u;
  if (lane == 0) g = atomicAdd(head, 1u);
  return (unsigned int)__builtin_amdgcn_readfirstlane((int)g);
}

// A wave's work counters into the call's, at the wave's exit (all lanes active): w holds the wave-uniform slots, slot
// `tests_slot` is the sum of the lanes' own triangle tests; one atomic add per non-zero slot, by lane 0
template <int SLOTS>
__device__ __forceinline__ void flush_counters(unsigned long long* stats, const unsigned long long (&w)[SLOTS], int tests_slot,
                                               unsigned long long lane_tests) {
  const unsigned long long tests = wave_sum(lane_tests);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < SLOTS; ++q) {
      const unsigned long long v = q == tests_slot ? tests : w[q];
      if (v) atomicAdd(&stats[q], v);
    }
  }
}

// The walk's closest hit h into the ray: set_hit (kernels.cl:198-201) on the arrays the walk read (P = the tiled copy, or the
// scene itself where the walk ran with BOXES = false).  No hit: the ray is left as it is.
__device__ __forceinline__ void finish_hit(const FrameParams& P, const TileHit& h, Ray& ray) {
  if (h.best < 0) return;
  const int j = h.best;
  const f3 v0 = xyz(P.verts[3 * j]), e1 = xyz(P.verts[3 * j + 1]) - v0, e2 = xyz(P.verts[3 * j + 2]) - v0;
  ray.tri = h.orig;
  ray.P = (v0 + h.u * e1) + h.v * e2;
  ray.N = xyz(P.normals[j]);
  ray.col = P.colors[j];
}

// ---- the tiled walk ----------------------------------------------------------------------------------------------------
constexpr int kQTile = 64;                  // triangles per tile of the tiled copy, for every kernel beside the frame's
                                            // (the mesh kernel keeps its own kTile: the same 64, the same copy)

// Step 1 of the walk, where the candidate tiles of a 64-tile pass come from, is a policy with one call:
//   cand_of(base, lane, ntiles, clear) -> 64-bit mask, the same in every lane: bit b = tile base + b is to be visited
// (clear(t): the walk's own bundle certificate says no ray of the wave can hit tile t; false where there is none.)
// The default asks it lane = tile.  The AOV pass (rt_aov.hip) brings the view's screen-cell masks instead.
struct BundleCandidates {
  template <class CLEAR>
  __device__ __forceinline__ unsigned long long operator()(int base, int lane, int ntiles, const CLEAR& clear) const {
    const int t = base + lane;
    return ballot(t < ntiles && !clear(t));
  }
};

// One lane = one ray (start o, direction d; SHADOW: radius_sq rsq) of a wave's 64, `act` = the lane has one; call with all
// 64 lanes.  P = the tiled copy (use_tiled_scene), tile = 4 * kQTile float4 of LDS that belong to this wave.
//   1. 64 tiles per pass, the candidate tiles of the pass from the policy `cand_of`.  BundleCandidates: the wave's rays bounded as one
//      bundle (bounce_bundle) against each tile's box, normal cone and sliver measure (tile_clear_for_bundle), lane = tile;
//   2. per candidate tile, the same certificate for each lane's own ray (es = ed = 0), ballot: no lane -> next tile;
//   3. the tile's records v0|material, e1|original index, e2, c = cof(e1, e2) are built into the wave's LDS from the tiled
//      copy, lane = triangle bounds the bundle (task_bound) and lane = ray tests the survivors with the reference's
//      arithmetic: closest hit carried across tiles in h with the original-order tie rule (closer), or (SHADOW) any-hit
//      into `blocked` with an early exit per lane and per wave.
// A ray outside in_query_domain takes every candidate tile and every triangle of it.  The spheres are the caller's.
// BOXES = false: P is a scene WITHOUT a tiled copy (n <= 64, RT_FLAG_GENERIC_KERNEL) — its triangles in their own order cut into
// runs of 64, no tile data: steps 1 and 2 pass every run, step 3 is the same.
// Counters (added to): rays outside the domain, (wave, tile) pairs that step 1 left, pairs whose triangles were tested
// (all three wave-uniform), and this LANE's triangle tests (the caller sums them over the wave: flush_counters).
template <bool SHADOW, bool BOXES = true, class CAND = BundleCandidates>
__device__ __forceinline__ void tile_walk(const FrameParams& P, float4* tile, int lane, bool act, f3 o, f3 d, float rsq,
                                          TileHit& h, bool& blocked, unsigned long long& n_unculled,
                                          unsigned long long& n_bundle_tiles, unsigned long long& n_tested_tiles,
                                          unsigned long long& lane_tests, const CAND& cand_of = CAND()) {
  float4* const tv0 = tile;                     // v0 | material
  float4* const te1 = tv0 + kQTile;             // e1 | original index
  float4* const te2 = tv0 + 2 * kQTile;         // e2
  float4* const tc = tv0 + 3 * kQTile;          // cof(e1, e2)
  const int n = P.n, ntiles = (n + kQTile - 1) / kQTile;
  const bool indom = act && in_query_domain(o, d);
  const bool brute = act && !indom;             // every tile, every triangle
  const unsigned long long brm = ballot(brute);
  n_unculled += __popcll(brm);
  // the wave's bundle (only while no lane is outside the domain: such a lane needs every tile anyway)
  const BounceBundle bnd = bounce_bundle(indom, o, d);
  const bool bundle_ok = brm == 0ull && bnd.mode == 1;
  const float d2 = 1.0001f * bsqrt(wave_max_pos(indom ? dot3(d, d) : 0.0f)) * 1.0001f;   // >= |d|_2 of every ray of the bundle
  const float dl = 1.0001f * bsqrt(dot3(d, d)) * 1.0001f;                               // >= |d|_2 of this lane's ray
  const f3 nd = -d;
  bool done = false;                            // SHADOW: every lane of the wave has found its blocker
  for (int base = 0; base < ntiles && !done; base += 64) {
    const unsigned long long cand = cand_of(base, lane, ntiles, [&](int t) {
      return BOXES && bundle_ok && tile_clear_for_bundle(P.tile_box + (size_t)3 * t, bnd.s0, bnd.D0, bnd.es, bnd.ed, d2);
    });
    n_bundle_tiles += __popcll(cand);
    for (unsigned long long m = uniform64(cand); m != 0ull; m &= m - 1ull) {
      const int tt = base + __builtin_ctzll(m);
      bool mine = act && !(SHADOW && blocked);
      if (BOXES && mine && !brute) mine = !tile_clear_for_bundle(P.tile_box + (size_t)3 * tt, o, d, 0.0f, 0.0f, dl);
      if (ballot(mine) == 0ull) continue;
      wave_lds_sync();                          // the previous tile's records are no longer read
      {
        const int gi = tt * kQTile + lane;
        if (gi < n) {
          const f3 v0 = xyz(P.verts[3 * gi]), e1 = xyz(P.verts[3 * gi + 1]) - v0, e2 = xyz(P.verts[3 * gi + 2]) - v0;
          const f3 cf = cof(e1, e2);
          tv0[lane] = make_float4(v0.x, v0.y, v0.z, P.colors[gi].w);
          te1[lane] = make_float4(e1.x, e1.y, e1.z, __int_as_float(BOXES ? P.orig[gi] : gi));
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
      n_tested_tiles += 1;
      if (mine) {
        // (uniform64: a loop inside a divergent `if` otherwise keeps its wave-uniform mask in vector registers)
        for (unsigned long long mm = uniform64(K); mm != 0ull; mm &= mm - 1ull) {
          const int i = __builtin_ctzll(mm);
          ++lane_tests;
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
}

constexpr int kScreenCell = 32;            // pixels per side of a screen cell of the primary-ray tile masks
constexpr int kScreenCellLog = 5;

}  // namespace
}  // namespace uobrt
