// rt_tiles.h — the exact tile certificate and the closest-hit tie rule of the tiled mesh copy, shared by the mesh kernel
// (rt_kernel_mesh.hip, bounce rays), the ray queries (rt_ray_query.hip) and the AOV pass (rt_aov.hip).  Include after rt_wave_common.h.
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
//   eta = max |e| / |e1 x e2| and emax = max |e| over the tile's triangles (rt_api.hip upload_tiled_scene).
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

// ---- shared by the ray queries (rt_ray_query.hip) and the AOV pass (rt_aov.hip) -----------------------------------------
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

constexpr int kScreenCell = 32;             // pixels per side of a screen cell of the primary-ray tile masks
constexpr int kScreenCellLog = 5;

}  // namespace
}  // namespace uobrt
