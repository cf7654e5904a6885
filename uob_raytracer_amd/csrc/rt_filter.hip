// rt_filter.hip — the edge-stopping a-trous filter of include/uob_rt.h ("rt_filter_plane") on the device, DESIGN.md 4.8a.
// A call is one guide-packing launch and one launch per pass.  The guides do not change between passes, so they are packed
// once into a 32-byte record per pixel (position.xyz | position.w, normal.xyz | pad): a tap then costs two aligned 16-byte
// loads and one 4-byte load instead of 36 bytes from three planes, and every acceptance test still sees the caller's FP32
// values.  A pass exists in two forms that compute the same bits:
//   tiled  (spacing s <= kFilterMaxTiledSpacing): a workgroup owns kFilterTX contiguous pixels of kFilterTY rows that are s
//           apart, stages those rows and two dilated rows either side, with 2 s pixels either side, in LDS, and takes all 25
//           taps from there: a record is fetched (TY+4)/TY * (TX+4s)/TX times per pass instead of 25 times;
//   direct (any spacing): a workgroup owns kFilterTX x kFilterTY adjacent pixels and takes its taps from the caches.
// One lane per pixel, the 25 taps in the defined order: the summation order is part of the contract.  host statement:
// filter_host.cpp.
#include "rt_host.h"

namespace uobrt {

namespace {

constexpr int TX = kFilterTX, TY = kFilterTY;          // one wave per row of the tile: 64 contiguous pixels
constexpr int kThreads = TX * TY;
static_assert(kThreads == 256, "slot_add sums four waves");
constexpr int kRowGroupsY = 32768;                      // row groups per grid.y; beyond that they continue in grid.z
enum { F_PIXELS = 0, F_PASSES = 1, F_TAPS = 2, F_VALID = 3, F_KEPT = 4 };
// Behind the eight exported counters: kCounterSlots partial sums of (accepted taps, kept, valid pixels), one 128-byte line each.  A
// workgroup adds to the slot of its index, so that a pass of 2^16 workgroups does not queue on one address (atomics on one
// address serialise); the last launch of a call sums the slots into the exported counters
constexpr int kCounterSlots = 64, kSlotWords = 16, kSlotBase = 8;

struct FilterArgs {
  int width, height;
  float normal_min_dot, plane_eps, vmax;                // vmax: value_max_diff * 2^-i of this pass
};

__device__ __forceinline__ float tap_weight(int dx, int dy) {
  const float h[3] = {0.375f, 0.25f, 0.0625f};
  return h[dx < 0 ? -dx : dx] * h[dy < 0 ? -dy : dy];
}

// The acceptance tests 1 (validity part) to 4 of a tap that lies inside the plane
__device__ __forceinline__ bool tap_accepted(const FilterArgs& a, const float4& Pp, const float4& Np, float vp, const float4& Pq,
                                             const float4& Nq, float vq) {
  if (!(Pq.w > 0.0f)) return false;
  const float nd = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;
  if (!(nd >= a.normal_min_dot)) return false;
  const float d0 = Pq.x - Pp.x, d1 = Pq.y - Pp.y, d2 = Pq.z - Pp.z;
  const float pd = (Np.x * d0 + Np.y * d1) + Np.z * d2;
  if (!(fabsf(pd) <= a.plane_eps)) return false;
  return fabsf(vq - vp) <= a.vmax;
}

// What a valid pixel stores: its own value when only the centre was accepted, else num / den (a NaN as the quiet NaN).
// A kept value keeps its BITS, a signalling NaN's payload included (the tests pin 0xFFA00001): vp reaches the store through
// moves only — loads, the LDS round trip in N.w, a select.  Do not route it through arithmetic, fminf / fmaxf or anything
// else that may quieten a NaN.
__device__ __forceinline__ float filtered_value(float num, float den, float vp) {
  if (den == 0.140625f) return vp;
  const float r = num / den;                            // correctly rounded (the compiler's IEEE division)
  return r == r ? r : __uint_as_float(0x7FC00000u);
}

__device__ __forceinline__ unsigned int wave_sum(unsigned int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// A workgroup of 256 adds its sum of `mine` (already summed per wave: lane 0 of each wave holds it) to word `word` of its
// slot: through LDS, one atomic per workgroup and counter (so at most one per wave and counter)
__device__ __forceinline__ void slot_add(unsigned long long* stats, unsigned int slot, int word, unsigned int wave_total) {
  __shared__ unsigned int s_count[3][4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_count[word][wave] = wave_total;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int total = (s_count[word][0] + s_count[word][1]) + (s_count[word][2] + s_count[word][3]);
    if (total) atomicAdd(&stats[kSlotBase + (slot & (kCounterSlots - 1)) * kSlotWords + word], (unsigned long long)total);
  }
}

__device__ __forceinline__ void flush_counters(unsigned long long* stats, bool valid, unsigned int taps, bool kept) {
  const unsigned int slot = blockIdx.x + blockIdx.y * 7u + blockIdx.z * 13u;
  slot_add(stats, slot, 0, wave_sum(valid ? taps : 0u));
  slot_add(stats, slot, 1, (unsigned int)__popcll(__ballot(valid && kept)));
}

// Behind the last pass: the slots into the exported counters
__global__ __launch_bounds__(64) void rt_filter_counters(unsigned long long* stats) {
  if (threadIdx.x != 0) return;
  unsigned long long sum[3] = {0, 0, 0};
  for (int k = 0; k < kCounterSlots; ++k)
    for (int w = 0; w < 3; ++w) sum[w] += stats[kSlotBase + k * kSlotWords + w];
  stats[F_TAPS] = sum[0];
  stats[F_KEPT] = sum[1];
  stats[F_VALID] = sum[2];
}

// The row group of this workgroup (grid.y, continued in grid.z), or -1 beyond the last
__device__ __forceinline__ long row_group(long groups) {
  const long g = (long)blockIdx.z * kRowGroupsY + blockIdx.y;
  return g < groups ? g : -1;
}

// position4 / normal4 -> the records, the count of valid pixels, and the call's constants among the counters
__global__ __launch_bounds__(256) void rt_filter_pack(const float4* __restrict__ pos, const float4* __restrict__ nrm, long count,
                                                      int passes, float4* __restrict__ rec, unsigned long long* stats) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  bool valid = false;
  if (p < count) {
    const float4 P = pos[p];
    const float4 N = nrm[p];
    rec[2 * p] = P;
    rec[2 * p + 1] = make_float4(N.x, N.y, N.z, 0.0f);
    valid = P.w > 0.0f;
  }
  slot_add(stats, blockIdx.x, 2, (unsigned int)__popcll(__ballot(valid)));
  if (p == 0) { stats[F_PIXELS] = (unsigned long long)count; stats[F_PASSES] = (unsigned long long)passes; }
}

// Direct form: adjacent rows, the taps from global memory
__global__ __launch_bounds__(kThreads) void rt_filter_direct(FilterArgs a, int s, long groups, const float4* __restrict__ rec,
                                                             const float* __restrict__ src, float* __restrict__ dst,
                                                             unsigned long long* stats) {
  const long g = row_group(groups);
  if (g < 0) return;
  const int lx = threadIdx.x & (TX - 1), ly = threadIdx.x / TX;
  const long x = (long)blockIdx.x * TX + lx, y = g * TY + ly;
  const bool inside = x < a.width && y < a.height;
  bool valid = false, kept = false;
  unsigned int taps = 0;
  if (inside) {
    const long c = y * a.width + x;
    const float vp = src[c];
    const float4 Pp = rec[2 * c], Np = rec[2 * c + 1];
    valid = Pp.w > 0.0f;
    float res = vp;
    if (valid) {
      float num = 0.0f, den = 0.0f;
#pragma unroll
      for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
          const float wt = tap_weight(dx, dy);
          bool take = dx == 0 && dy == 0;
          float vq = vp;
          if (!take) {
            const long qx = x + (long)dx * s, qy = y + (long)dy * s;
            if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
              const long q = qy * a.width + qx;
              vq = src[q];
              take = tap_accepted(a, Pp, Np, vp, rec[2 * q], rec[2 * q + 1], vq);
            }
          }
          if (take) { num = num + wt * vq; den = den + wt; ++taps; }
        }
      kept = den == 0.140625f;
      res = filtered_value(num, den, vp);
    }
    dst[c] = res;                                       // (an invalid or kept pixel: vp's own bits, see filtered_value)
  }
  flush_counters(stats, valid, taps, kept);
}

// Tiled form at the compile-time spacing S: rows y = r + (k*TY + j) * S of the residue class r = group / per_class
template <int S>
__global__ __launch_bounds__(kThreads) void rt_filter_tiled(FilterArgs a, long per_class, long groups, const float4* __restrict__ rec,
                                                            const float* __restrict__ src, float* __restrict__ dst,
                                                            unsigned long long* stats) {
  constexpr int W = TX + 4 * S, R = TY + 4;
  __shared__ float4 s_pos[R][W];                        // position.xyz | position.w (0: outside the plane)
  __shared__ float4 s_nv[R][W];                         // normal.xyz | the value
  const long g = row_group(groups);
  if (g < 0) return;
  const long r = g / per_class, k = g - r * per_class;
  if (r >= a.height) return;                            // (S beyond the height: the classes r >= height are empty)
  const long x0 = (long)blockIdx.x * TX, y0 = r + k * TY * S;
  for (int i = threadIdx.x; i < R * W; i += kThreads) {
    const int row = i / W, col = i - row * W;
    const long qx = x0 - 2 * S + col, qy = y0 + (long)(row - 2) * S;
    float4 P = make_float4(0.f, 0.f, 0.f, 0.f), N = P;
    if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
      const long q = qy * a.width + qx;
      P = rec[2 * q];
      N = rec[2 * q + 1];
      N.w = src[q];
    }
    s_pos[row][col] = P;
    s_nv[row][col] = N;
  }
  __syncthreads();
  const int lx = threadIdx.x & (TX - 1), ly = threadIdx.x / TX;
  const long x = x0 + lx, y = y0 + (long)ly * S;
  const bool inside = x < a.width && y < a.height;
  bool valid = false, kept = false;
  unsigned int taps = 0;
  if (inside) {
    const float4 Pp = s_pos[ly + 2][lx + 2 * S], Np = s_nv[ly + 2][lx + 2 * S];
    const float vp = Np.w;
    valid = Pp.w > 0.0f;
    float res = vp;
    if (valid) {
      float num = 0.0f, den = 0.0f;
#pragma unroll
      for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
          const float wt = tap_weight(dx, dy);
          bool take = dx == 0 && dy == 0;
          float vq = vp;
          if (!take) {
            const float4 Pq = s_pos[ly + 2 + dy][lx + (2 + dx) * S], Nq = s_nv[ly + 2 + dy][lx + (2 + dx) * S];
            vq = Nq.w;
            take = tap_accepted(a, Pp, Np, vp, Pq, Nq, vq);   // (a slot outside the plane has w = 0)
          }
          if (take) { num = num + wt * vq; den = den + wt; ++taps; }
        }
      kept = den == 0.140625f;
      res = filtered_value(num, den, vp);
    }
    dst[y * a.width + x] = res;                         // (an invalid or kept pixel: vp's own bits, see filtered_value)
  }
  flush_counters(stats, valid, taps, kept);
}

template <int S>
void launch_tiled(const FilterArgs& a, dim3 grid, long per_class, long groups, const float4* rec, const float* src, float* dst,
                  unsigned long long* stats, hipStream_t stream) {
  hipLaunchKernelGGL(rt_filter_tiled<S>, grid, dim3(kThreads), 0, stream, a, per_class, groups, rec, src, dst, stats);
}

}  // namespace

int filter_stats_words() { return kSlotBase + kCounterSlots * kSlotWords; }

void launch_filter_counters(unsigned long long* stats, hipStream_t stream) {
  hipLaunchKernelGGL(rt_filter_counters, dim3(1), dim3(64), 0, stream, stats);
}

void launch_filter_pack(const float4* d_pos, const float4* d_nrm, long count, int passes, float4* d_rec, unsigned long long* stats,
                        hipStream_t stream) {
  hipLaunchKernelGGL(rt_filter_pack, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, d_pos, d_nrm, count, passes,
                     d_rec, stats);
}

static bool filter_pass_is_tiled(int pass, int form) {
  return form != kFilterFormDirect && (1 << pass) <= kFilterMaxTiledSpacing;
}

void launch_filter_pass(const rt_filter_params& p, int pass, int form, const float4* d_rec, const float* d_src, float* d_dst,
                        unsigned long long* stats, hipStream_t stream) {
  const int s = 1 << pass;
  const FilterArgs a{p.width, p.height, p.normal_min_dot, p.plane_eps, p.value_max_diff * ldexpf(1.0f, -pass)};
  const unsigned tiles_x = (unsigned)(((long)p.width + TX - 1) / TX);
  const bool tiled = filter_pass_is_tiled(pass, form);
  // tiled: s residue classes of ceil(ceil(height / s) / TY) groups each; direct: ceil(height / TY) groups of adjacent rows
  const long per_class = tiled ? (((long)p.height + s - 1) / s + TY - 1) / TY : 0;
  const long groups = tiled ? per_class * s : ((long)p.height + TY - 1) / TY;
  const dim3 grid(tiles_x, (unsigned)(groups < kRowGroupsY ? groups : kRowGroupsY), (unsigned)((groups + kRowGroupsY - 1) / kRowGroupsY));
  if (!tiled) {
    hipLaunchKernelGGL(rt_filter_direct, grid, dim3(kThreads), 0, stream, a, s, groups, d_rec, d_src, d_dst, stats);
    return;
  }
  switch (s) {
    case 1: launch_tiled<1>(a, grid, per_class, groups, d_rec, d_src, d_dst, stats, stream); break;
    case 2: launch_tiled<2>(a, grid, per_class, groups, d_rec, d_src, d_dst, stats, stream); break;
    case 4: launch_tiled<4>(a, grid, per_class, groups, d_rec, d_src, d_dst, stats, stream); break;
    case 8: launch_tiled<8>(a, grid, per_class, groups, d_rec, d_src, d_dst, stats, stream); break;
    case 16: launch_tiled<16>(a, grid, per_class, groups, d_rec, d_src, d_dst, stats, stream); break;
    default: launch_tiled<32>(a, grid, per_class, groups, d_rec, d_src, d_dst, stats, stream); break;
  }
}

}  // namespace uobrt
