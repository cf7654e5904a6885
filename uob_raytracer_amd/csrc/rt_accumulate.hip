// rt_accumulate.hip — the temporal reprojection of include/uob_rt.h ("rt_accumulate_plane") on the device, DESIGN.md 4.8b.
// A call is one launch over the plane and a one-wave launch that sums the counters.  One lane per pixel; a workgroup of 256
// owns kFilterTX x kFilterTY adjacent pixels, one wave per row: neighbouring pixels reproject to neighbouring places, so the
// four taps of a wave fall on two runs of about 65 consecutive 48-byte records, and vertically neighbouring waves share
// their rows in the CU's cache.  A history record is three 16-byte loads, and three 16-byte stores when it is written.  The
// taps are taken in the defined order: the summation order is part of the contract.  host statement: accumulate_host.cpp.
// rt_accumulate_plane_moving is the same kernel with the reprojection planes in place of the guides in the projection and the
// two geometric tests (two more 16-byte loads per pixel): the instantiation without them is the plain entry's code.
#include "rt_host.h"

namespace uobrt {

namespace {

constexpr int TX = kFilterTX, TY = kFilterTY;          // one wave per row of the tile: 64 contiguous pixels
constexpr int kThreads = TX * TY;
static_assert(kThreads == 256, "flush_counters sums four waves");
constexpr int kRowGroupsY = 32768;                      // row groups per grid.y; beyond that they continue in grid.z
enum { A_PIXELS = 0, A_VALID = 1, A_FOUND = 2, A_TAPS = 3, A_NOCAND = 4 };
// Behind the eight exported counters: kCounterSlots partial sums of (valid, found, taps, no candidate), one 128-byte line
// each.  A workgroup adds to the slot of its index, so that 2^16 workgroups do not queue on one address (atomics on one
// address serialise); the last launch of a call sums the slots into the exported counters
constexpr int kCounterSlots = 64, kSlotWords = 16, kSlotBase = 8, kCounters = 4;

struct AccumulateArgs {
  rt_accumulate_params p;
  long groups;
  const float* value;
  const float4* pos;
  const float4* nrm;
  const int* prim;
  const float4* rpos;              // the reprojection planes (kReproj instantiation only)
  const float4* rnrm;
  const float4* prev;
  float4* next;
  float* out_mean;
  float* out_variance;
};

__device__ __forceinline__ float quiet_if_nan(float v) { return v == v ? v : __uint_as_float(0x7FC00000u); }

__device__ __forceinline__ unsigned int wave_sum(unsigned int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// The workgroup's sums of the four counters into its slot: lanes per wave, waves through LDS, one atomic per counter
__device__ __forceinline__ void flush_counters(unsigned long long* stats, bool valid, bool found, unsigned int taps, bool nocand) {
  __shared__ unsigned int s_count[kCounters][4];
  const unsigned int mine[kCounters] = {(unsigned int)__popcll(__ballot(valid)), (unsigned int)__popcll(__ballot(found)), wave_sum(taps),
                                        (unsigned int)__popcll(__ballot(nocand))};
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < kCounters; ++k) s_count[k][wave] = mine[k];
  __syncthreads();
  if (threadIdx.x < kCounters) {
    const int k = threadIdx.x;
    const unsigned int total = (s_count[k][0] + s_count[k][1]) + (s_count[k][2] + s_count[k][3]);
    const unsigned int slot = (blockIdx.x + blockIdx.y * 7u + blockIdx.z * 13u) & (kCounterSlots - 1);
    if (total) atomicAdd(&stats[kSlotBase + slot * kSlotWords + k], (unsigned long long)total);
  }
}

// Behind the plane's launch: the slots into the exported counters
__global__ __launch_bounds__(64) void rt_accumulate_counters(unsigned long long* stats, long pixels) {
  if (threadIdx.x != 0) return;
  unsigned long long sum[kCounters] = {0, 0, 0, 0};
  for (int s = 0; s < kCounterSlots; ++s)
    for (int k = 0; k < kCounters; ++k) sum[k] += stats[kSlotBase + s * kSlotWords + k];
  stats[A_PIXELS] = (unsigned long long)pixels;
  stats[A_VALID] = sum[0];
  stats[A_FOUND] = sum[1];
  stats[A_TAPS] = sum[2];
  stats[A_NOCAND] = sum[3];
}

template <bool kReproj>
__global__ __launch_bounds__(kThreads) void rt_accumulate_pixels(AccumulateArgs a, unsigned long long* stats) {
  const long g = (long)blockIdx.z * kRowGroupsY + blockIdx.y;
  if (g >= a.groups) return;                            // (the whole workgroup: beyond the last row group)
  const rt_accumulate_params& p = a.p;
  const int lx = threadIdx.x & (TX - 1), ly = threadIdx.x / TX;
  const long w = p.width, h = p.height;
  const long x = (long)blockIdx.x * TX + lx, y = g * TY + ly;
  bool valid = false, nocand = false;
  unsigned int taps = 0;
  if (x < w && y < h) {
    const long c = y * w + x;
    const float v = a.value[c];
    const float4 P = a.pos[c], N = a.nrm[c];
    const int pr = a.prim ? a.prim[c] : -1;
    const float vv = v * v;
    valid = P.w > 0.0f;
    float num = 0.0f, num2 = 0.0f, den = 0.0f, cmin = __builtin_inff();
    if (valid && a.prev) {
      const float* rot = p.prev_rot;
      // what is projected and tested against the records: the guides, or where the surface point was then (Pr.w > 0: it was)
      float4 Pr = P, Nr = N;
      if constexpr (kReproj) { Pr = a.rpos[c]; Nr = a.rnrm[c]; }
      const float d0 = Pr.x - p.prev_cam[0], d1 = Pr.y - p.prev_cam[1], d2 = Pr.z - p.prev_cam[2];
      const float q0 = (d0 * rot[0] + d1 * rot[4]) + d2 * rot[8];
      const float q1 = (d0 * rot[1] + d1 * rot[5]) + d2 * rot[9];
      const float q2 = (d0 * rot[2] + d1 * rot[6]) + d2 * rot[10];
      const float fx = (q0 * p.prev_focal_px) / q2 + 0.5f * (float)p.width;   // correctly rounded (the compiler's IEEE division)
      const float fy = (q1 * p.prev_focal_px) / q2 + 0.5f * (float)p.height;
      nocand = !(q2 > 0.0f && fx >= -1.0f && fx < (float)p.width && fy >= -1.0f && fy < (float)p.height);
      if constexpr (kReproj) nocand = nocand || !(Pr.w > 0.0f);
      if (!nocand) {
        const float xf = floorf(fx), yf = floorf(fy);
        const float ax = fx - xf, ay = fy - yf;
        const long x0 = (long)xf, y0 = (long)yf;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const long qx = x0 + i, qy = y0 + j;
            const float wt = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
            if (qx < 0 || qx >= w || qy < 0 || qy >= h || !(wt > 0.0f)) continue;   // (no record outside the plane is read)
            const float4* r = a.prev + 3 * (qy * w + qx);
            const float4 r0 = r[0], r1 = r[1], r2 = r[2];   // position | mean, normal | m2, count | prim | pad
            if (!(r2.x > 0.0f)) continue;
            if (a.prim && __float_as_int(r2.y) != pr) continue;
            const float nd = (Nr.x * r1.x + Nr.y * r1.y) + Nr.z * r1.z;
            if (!(nd >= p.normal_min_dot)) continue;
            const float e0 = r0.x - Pr.x, e1 = r0.y - Pr.y, e2 = r0.z - Pr.z;
            const float pd = (Nr.x * e0 + Nr.y * e1) + Nr.z * e2;
            if (!(fabsf(pd) <= p.plane_eps)) continue;
            num = num + wt * r0.w;
            num2 = num2 + wt * r1.w;
            den = den + wt;
            cmin = r2.x < cmin ? r2.x : cmin;
            ++taps;
          }
      }
    }
    // A first frame keeps the value's BITS, a signalling NaN's payload included: v reaches the store through moves only —
    // the load and a select.  Do not route it through arithmetic, fminf / fmaxf or anything else that may quieten a NaN.
    float mean = v, m2 = quiet_if_nan(vv), count = valid ? 1.0f : 0.0f;
    if (taps != 0) {
      const float mp = num / den, sp = num2 / den;
      const float nmax = (float)(p.max_history - 1);
      const float n = (cmin < nmax ? cmin : nmax) + 1.0f;
      const float s = 1.0f / n;
      const float t1 = v - mp;
      mean = quiet_if_nan(mp + s * t1);
      const float t2 = vv - sp;
      m2 = quiet_if_nan(sp + s * t2);
      count = n;
    }
    float4* o = a.next + 3 * c;
    o[0] = make_float4(P.x, P.y, P.z, mean);
    o[1] = make_float4(N.x, N.y, N.z, m2);
    o[2] = make_float4(count, __int_as_float(pr), 0.0f, 0.0f);
    if (a.out_mean) a.out_mean[c] = mean;
    if (a.out_variance) {
      const float t = m2 - mean * mean;
      a.out_variance[c] = t > 0.0f ? t : 0.0f;
    }
  }
  flush_counters(stats, valid, taps != 0, taps, valid && nocand);
}

}  // namespace

int accumulate_stats_words() { return kSlotBase + kCounterSlots * kSlotWords; }

void launch_accumulate(const rt_accumulate_params& p, const float* d_value, const float4* d_pos, const float4* d_nrm, const int* d_prim,
                       const float4* d_rpos, const float4* d_rnrm, const float4* d_prev, float4* d_next, float* d_out_mean,
                       float* d_out_variance, unsigned long long* stats, hipStream_t stream) {
  const unsigned tiles_x = (unsigned)(((long)p.width + TX - 1) / TX);
  const long groups = ((long)p.height + TY - 1) / TY;
  const dim3 grid(tiles_x, (unsigned)(groups < kRowGroupsY ? groups : kRowGroupsY), (unsigned)((groups + kRowGroupsY - 1) / kRowGroupsY));
  const AccumulateArgs a{p, groups, d_value, d_pos, d_nrm, d_prim, d_rpos, d_rnrm, d_prev, d_next, d_out_mean, d_out_variance};
  if (d_rpos)
    hipLaunchKernelGGL(rt_accumulate_pixels<true>, grid, dim3(kThreads), 0, stream, a, stats);
  else
    hipLaunchKernelGGL(rt_accumulate_pixels<false>, grid, dim3(kThreads), 0, stream, a, stats);
  hipLaunchKernelGGL(rt_accumulate_counters, dim3(1), dim3(64), 0, stream, stats, (long)p.width * p.height);
}

}  // namespace uobrt
