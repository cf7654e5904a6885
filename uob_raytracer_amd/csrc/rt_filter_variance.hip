// rt_filter_variance.hip — the variance-guided a-trous filter of include/uob_rt.h ("rt_filter_plane_variance") on the device,
// DESIGN.md 4.8a'.  A call is rt_filter.hip's guide-packing launch and two launches per pass:
//   threshold: T = sigma_value * sqrt(3 x 3 blur of the variance at spacing 1) + value_eps, one float per pixel, validity
//              from the records' position.w;
//   a-trous:   rt_filter.hip's pass with test 5 (|dv| <= T of the centre) and the variance plane carried beside the value,
//              in the same two forms that compute the same bits:
//     tiled  (spacing s <= kFilterVarianceMaxTiledSpacing): the tile of rt_filter.hip, with a third LDS plane for the variance
//             (36 bytes per slot; at s = 32 that is 8 x 192 x 36 = 55 296 bytes, two workgroups per CU);
//     direct (any spacing): kFilterTX x kFilterTY adjacent pixels, the taps from the caches.
// One lane per pixel, the 25 taps in the defined order: the summation order is part of the contract.  The counters use the
// slots of rt_filter.hip (filter_stats_words), with a fourth word per slot for the taps that only test 5 stopped.  host
// statement: filter_variance_host.cpp.
#include "rt_host.h"

namespace uobrt {

namespace {

constexpr int TX = kFilterTX, TY = kFilterTY;          // one wave per row of the tile: 64 contiguous pixels
constexpr int kThreads = TX * TY;
static_assert(kThreads == 256, "slot_add sums four waves");
constexpr int kRowGroupsY = 32768;                      // row groups per grid.y; beyond that they continue in grid.z
// rt_filter.hip's layout of the counters: 8 exported words, then kCounterSlots lines of kSlotWords; words 0 .. 2 of a slot
// are its (accepted taps, kept, valid pixels), word 3 is this file's (taps stopped by test 5 alone)
enum { F_TAPS = 2, F_VALID = 3, F_KEPT = 4, F_STOPPED = 5 };
constexpr int kCounterSlots = 64, kSlotWords = 16, kSlotBase = 8;
constexpr int kCounters = 4;

struct VarianceArgs {
  int width, height;
  float normal_min_dot, plane_eps, vmax;                // vmax: value_max_diff * 2^-i of this pass
};

__device__ __forceinline__ float tap_weight(int dx, int dy) {
  const float h[3] = {0.375f, 0.25f, 0.0625f};
  return h[dx < 0 ? -dx : dx] * h[dy < 0 ? -dy : dy];
}

// The acceptance tests 1 (validity part) to 4 of a tap that lies inside the plane; dv = fabsf(vq - vp)
__device__ __forceinline__ bool tap_passes_four(const VarianceArgs& a, const float4& Pp, const float4& Np, const float4& Pq,
                                                const float4& Nq, float dv) {
  if (!(Pq.w > 0.0f)) return false;
  const float nd = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;
  if (!(nd >= a.normal_min_dot)) return false;
  const float d0 = Pq.x - Pp.x, d1 = Pq.y - Pp.y, d2 = Pq.z - Pp.z;
  const float pd = (Np.x * d0 + Np.y * d1) + Np.z * d2;
  if (!(fabsf(pd) <= a.plane_eps)) return false;
  return dv <= a.vmax;
}

// What a pixel that was not kept stores: the quotient, a NaN as the quiet NaN.  A kept pixel never comes here: its value and
// its variance reach the store through moves only (loads, the LDS round trip, a select), so that they keep their bits
__device__ __forceinline__ float quotient(float num, float den) {
  const float r = num / den;                            // correctly rounded (the compiler's IEEE division)
  return r == r ? r : __uint_as_float(0x7FC00000u);
}

__device__ __forceinline__ unsigned int wave_sum(unsigned int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// A workgroup of 256 adds its sum of `mine` (already summed per wave: lane 0 of each wave holds it) to word `word` of its
// slot: through LDS, one atomic per workgroup and counter
__device__ __forceinline__ void slot_add(unsigned long long* stats, unsigned int slot, int word, unsigned int wave_total) {
  __shared__ unsigned int s_count[kCounters][4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_count[word][wave] = wave_total;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int total = (s_count[word][0] + s_count[word][1]) + (s_count[word][2] + s_count[word][3]);
    if (total) atomicAdd(&stats[kSlotBase + (slot & (kCounterSlots - 1)) * kSlotWords + word], (unsigned long long)total);
  }
}

__device__ __forceinline__ void flush_counters(unsigned long long* stats, bool valid, unsigned int taps, bool kept,
                                               unsigned int stopped) {
  const unsigned int slot = blockIdx.x + blockIdx.y * 7u + blockIdx.z * 13u;
  slot_add(stats, slot, 0, wave_sum(valid ? taps : 0u));
  slot_add(stats, slot, 1, (unsigned int)__popcll(__ballot(valid && kept)));
  slot_add(stats, slot, 3, wave_sum(valid ? stopped : 0u));
}

// Behind the last pass: the slots into the exported counters (word 2, the valid pixels, is the packing launch's)
__global__ __launch_bounds__(64) void rt_filter_variance_counters(unsigned long long* stats) {
  if (threadIdx.x != 0) return;
  unsigned long long sum[kCounters] = {0, 0, 0, 0};
  for (int k = 0; k < kCounterSlots; ++k)
    for (int w = 0; w < kCounters; ++w) sum[w] += stats[kSlotBase + k * kSlotWords + w];
  stats[F_TAPS] = sum[0];
  stats[F_KEPT] = sum[1];
  stats[F_VALID] = sum[2];
  stats[F_STOPPED] = sum[3];
}

// The row group of this workgroup (grid.y, continued in grid.z), or -1 beyond the last
__device__ __forceinline__ long row_group(long groups) {
  const long g = (long)blockIdx.z * kRowGroupsY + blockIdx.y;
  return g < groups ? g : -1;
}

// The value stop of a pass: kFilterTX x kFilterTY adjacent pixels per workgroup, the 9 taps from the caches
__global__ __launch_bounds__(kThreads) void rt_filter_variance_threshold(int width, int height, float sigma, float eps, long groups,
                                                                         const float4* __restrict__ rec,
                                                                         const float* __restrict__ var, float* __restrict__ T) {
  const long g = row_group(groups);
  if (g < 0) return;
  const int lx = threadIdx.x & (TX - 1), ly = threadIdx.x / TX;
  const long x = (long)blockIdx.x * TX + lx, y = g * TY + ly;
  if (x >= width || y >= height) return;
  const long c = y * width + x;
  if (!(rec[2 * c].w > 0.0f)) { T[c] = 0.0f; return; }   // (never read: an invalid pixel takes no taps)
  const float vc = var[c];
  float sum = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const float k = (dx != 0 && dy != 0) ? 0.0625f : (dx != 0 || dy != 0) ? 0.125f : 0.25f;
      float cv = vc;
      if (dx != 0 || dy != 0) {
        const long qx = x + dx, qy = y + dy;
        if (qx >= 0 && qx < width && qy >= 0 && qy < height) {
          const long q = qy * width + qx;
          if (rec[2 * q].w > 0.0f) cv = var[q];
        }
      }
      sum = sum + k * cv;
    }
  T[c] = sigma * sqrtf(sum) + eps;                       // sqrtf: correctly rounded (rt_math.h)
}

// Direct form: adjacent rows, the taps from global memory
__global__ __launch_bounds__(kThreads) void rt_filter_variance_direct(VarianceArgs a, int s, long groups, const float4* __restrict__ rec,
                                                                      const float* __restrict__ T, const float* __restrict__ src,
                                                                      const float* __restrict__ vsrc, float* __restrict__ dst,
                                                                      float* __restrict__ vdst, unsigned long long* stats) {
  const long g = row_group(groups);
  if (g < 0) return;
  const int lx = threadIdx.x & (TX - 1), ly = threadIdx.x / TX;
  const long x = (long)blockIdx.x * TX + lx, y = g * TY + ly;
  const bool inside = x < a.width && y < a.height;
  bool valid = false, kept = false;
  unsigned int taps = 0, stopped = 0;
  if (inside) {
    const long c = y * a.width + x;
    const float vp = src[c], varp = vsrc[c];
    const float4 Pp = rec[2 * c], Np = rec[2 * c + 1];
    valid = Pp.w > 0.0f;
    float res = vp, res2 = varp;
    if (valid) {
      const float t = T[c];
      float num = 0.0f, den = 0.0f, num2 = 0.0f;
#pragma unroll
      for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
          const float wt = tap_weight(dx, dy);
          bool take = dx == 0 && dy == 0;
          float vq = vp, varq = varp;
          if (!take) {
            const long qx = x + (long)dx * s, qy = y + (long)dy * s;
            if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
              const long q = qy * a.width + qx;
              vq = src[q];
              const float dv = fabsf(vq - vp);
              if (tap_passes_four(a, Pp, Np, rec[2 * q], rec[2 * q + 1], dv)) {
                take = dv <= t;
                if (take) varq = vsrc[q]; else ++stopped;
              }
            }
          }
          if (take) { num = num + wt * vq; den = den + wt; num2 = num2 + (wt * wt) * varq; ++taps; }
        }
      kept = den == 0.140625f;
      if (!kept) { res = quotient(num, den); res2 = quotient(num2, den * den); }
    }
    dst[c] = res;                                       // (an invalid or kept pixel: the bits of vp and varp)
    vdst[c] = res2;
  }
  flush_counters(stats, valid, taps, kept, stopped);
}

// Tiled form at the compile-time spacing S: rows y = r + (k*TY + j) * S of the residue class r = group / per_class
template <int S>
__global__ __launch_bounds__(kThreads) void rt_filter_variance_tiled(VarianceArgs a, long per_class, long groups,
                                                                     const float4* __restrict__ rec, const float* __restrict__ T,
                                                                     const float* __restrict__ src, const float* __restrict__ vsrc,
                                                                     float* __restrict__ dst, float* __restrict__ vdst,
                                                                     unsigned long long* stats) {
  constexpr int W = TX + 4 * S, R = TY + 4;
  __shared__ float4 s_pos[R][W];                        // position.xyz | position.w (0: outside the plane)
  __shared__ float4 s_nv[R][W];                         // normal.xyz | the value
  __shared__ float s_var[R][W];                         // the variance
  static_assert(sizeof(float) * 9 * R * W + 64 <= 65536, "the tile of this spacing does not fit the LDS of a workgroup");
  const long g = row_group(groups);
  if (g < 0) return;
  const long r = g / per_class, k = g - r * per_class;
  if (r >= a.height) return;                            // (S beyond the height: the classes r >= height are empty)
  const long x0 = (long)blockIdx.x * TX, y0 = r + k * TY * S;
  for (int i = threadIdx.x; i < R * W; i += kThreads) {
    const int row = i / W, col = i - row * W;
    const long qx = x0 - 2 * S + col, qy = y0 + (long)(row - 2) * S;
    float4 P = make_float4(0.f, 0.f, 0.f, 0.f), N = P;
    float v2 = 0.0f;
    if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
      const long q = qy * a.width + qx;
      P = rec[2 * q];
      N = rec[2 * q + 1];
      N.w = src[q];
      v2 = vsrc[q];
    }
    s_pos[row][col] = P;
    s_nv[row][col] = N;
    s_var[row][col] = v2;
  }
  __syncthreads();
  const int lx = threadIdx.x & (TX - 1), ly = threadIdx.x / TX;
  const long x = x0 + lx, y = y0 + (long)ly * S;
  const bool inside = x < a.width && y < a.height;
  bool valid = false, kept = false;
  unsigned int taps = 0, stopped = 0;
  if (inside) {
    const float4 Pp = s_pos[ly + 2][lx + 2 * S], Np = s_nv[ly + 2][lx + 2 * S];
    const float vp = Np.w, varp = s_var[ly + 2][lx + 2 * S];
    valid = Pp.w > 0.0f;
    float res = vp, res2 = varp;
    if (valid) {
      const float t = T[y * a.width + x];
      float num = 0.0f, den = 0.0f, num2 = 0.0f;
#pragma unroll
      for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
          const float wt = tap_weight(dx, dy);
          bool take = dx == 0 && dy == 0;
          float vq = vp, varq = varp;
          if (!take) {
            const float4 Pq = s_pos[ly + 2 + dy][lx + (2 + dx) * S], Nq = s_nv[ly + 2 + dy][lx + (2 + dx) * S];
            vq = Nq.w;
            const float dv = fabsf(vq - vp);
            if (tap_passes_four(a, Pp, Np, Pq, Nq, dv)) {   // (a slot outside the plane has w = 0)
              take = dv <= t;
              if (take) varq = s_var[ly + 2 + dy][lx + (2 + dx) * S]; else ++stopped;
            }
          }
          if (take) { num = num + wt * vq; den = den + wt; num2 = num2 + (wt * wt) * varq; ++taps; }
        }
      kept = den == 0.140625f;
      if (!kept) { res = quotient(num, den); res2 = quotient(num2, den * den); }
    }
    dst[y * a.width + x] = res;                         // (an invalid or kept pixel: the bits of vp and varp)
    vdst[y * a.width + x] = res2;
  }
  flush_counters(stats, valid, taps, kept, stopped);
}

template <int S>
void launch_tiled(const VarianceArgs& a, dim3 grid, long per_class, long groups, const float4* rec, const float* T, const float* src,
                  const float* vsrc, float* dst, float* vdst, unsigned long long* stats, hipStream_t stream) {
  static_assert(S <= kFilterVarianceMaxTiledSpacing, "a tiled spacing beyond the largest");
  hipLaunchKernelGGL(rt_filter_variance_tiled<S>, grid, dim3(kThreads), 0, stream, a, per_class, groups, rec, T, src, vsrc, dst, vdst,
                     stats);
}

// The grid of a launch over `groups` row groups
dim3 grid_for(int width, long groups) {
  const unsigned tiles_x = (unsigned)(((long)width + TX - 1) / TX);
  return dim3(tiles_x, (unsigned)(groups < kRowGroupsY ? groups : kRowGroupsY), (unsigned)((groups + kRowGroupsY - 1) / kRowGroupsY));
}

}  // namespace

void launch_filter_variance_counters(unsigned long long* stats, hipStream_t stream) {
  hipLaunchKernelGGL(rt_filter_variance_counters, dim3(1), dim3(64), 0, stream, stats);
}

void launch_filter_variance_threshold(const rt_filter_variance_params& vp, const float4* d_rec, const float* d_var, float* d_T,
                                      hipStream_t stream) {
  const long groups = ((long)vp.base.height + TY - 1) / TY;
  hipLaunchKernelGGL(rt_filter_variance_threshold, grid_for(vp.base.width, groups), dim3(kThreads), 0, stream, vp.base.width,
                     vp.base.height, vp.sigma_value, vp.value_eps, groups, d_rec, d_var, d_T);
}

void launch_filter_variance_pass(const rt_filter_variance_params& vp, int pass, int form, const float4* d_rec, const float* d_T,
                                 const float* d_src, const float* d_vsrc, float* d_dst, float* d_vdst, unsigned long long* stats,
                                 hipStream_t stream) {
  const rt_filter_params& p = vp.base;
  const int s = 1 << pass;
  const VarianceArgs a{p.width, p.height, p.normal_min_dot, p.plane_eps, p.value_max_diff * ldexpf(1.0f, -pass)};
  const bool tiled = form != kFilterFormDirect && s <= kFilterVarianceMaxTiledSpacing;
  // tiled: s residue classes of ceil(ceil(height / s) / TY) groups each; direct: ceil(height / TY) groups of adjacent rows
  const long per_class = tiled ? (((long)p.height + s - 1) / s + TY - 1) / TY : 0;
  const long groups = tiled ? per_class * s : ((long)p.height + TY - 1) / TY;
  const dim3 grid = grid_for(p.width, groups);
  if (!tiled) {
    hipLaunchKernelGGL(rt_filter_variance_direct, grid, dim3(kThreads), 0, stream, a, s, groups, d_rec, d_T, d_src, d_vsrc, d_dst, d_vdst,
                       stats);
    return;
  }
  switch (s) {
    case 1: launch_tiled<1>(a, grid, per_class, groups, d_rec, d_T, d_src, d_vsrc, d_dst, d_vdst, stats, stream); break;
    case 2: launch_tiled<2>(a, grid, per_class, groups, d_rec, d_T, d_src, d_vsrc, d_dst, d_vdst, stats, stream); break;
    case 4: launch_tiled<4>(a, grid, per_class, groups, d_rec, d_T, d_src, d_vsrc, d_dst, d_vdst, stats, stream); break;
    case 8: launch_tiled<8>(a, grid, per_class, groups, d_rec, d_T, d_src, d_vsrc, d_dst, d_vdst, stats, stream); break;
    case 16: launch_tiled<16>(a, grid, per_class, groups, d_rec, d_T, d_src, d_vsrc, d_dst, d_vdst, stats, stream); break;
    default: launch_tiled<32>(a, grid, per_class, groups, d_rec, d_T, d_src, d_vsrc, d_dst, d_vdst, stats, stream); break;
  }
}

}  // namespace uobrt
