// rt_selftest.hip — on-device self tests of the numerics building blocks (C ABI: rt_selftest_rcp, rt_selftest_normalize,
// rt_selftest_shade, rt_selftest_all_within).
#include <hip/hip_runtime.h>

#include "rt_host.h"
#include "rt_math.h"
#include "rt_wave_common.h"

namespace uobrt {

// For every FP32 bit pattern x: compare the Newton-refined v_rcp_f32 (1 and 2 steps) with the correctly
// rounded 1.0f/x.  out[0]/out[1]: mismatches of the 1-/2-step form over the "safe" magnitudes
// 2^-100 <= |x| <= 2^100 (far from the flush/overflow ends); out[2]/out[3]: mismatches over every other
// finite non-zero x; out[4]: number of recorded examples; out[8..]: up to 56 mismatching patterns of
// the 1-step form inside the safe range (low 32 bits = x).
__global__ __launch_bounds__(256) void k_selftest_rcp(unsigned long long* out) {
  const unsigned long long total = 1ull << 32;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  unsigned long long bad1 = 0, bad2 = 0, obad1 = 0, obad2 = 0;
  for (unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += stride) {
    const uint32_t bits = (uint32_t)k;
    const float x = __uint_as_float(bits);
    const uint32_t mag = bits & 0x7fffffffu;
    if (mag == 0u || mag >= 0x7f800000u) continue;   // zero, inf, NaN
    const float ref = 1.0f / x;
    const float r1 = rcp_newton(x, 1), r2 = rcp_newton(x, 2);
    const bool safe = mag >= 0x0d800000u && mag <= 0x71800000u;   // 2^-100 .. 2^100
    const bool m1 = __float_as_uint(r1) != __float_as_uint(ref);
    const bool m2 = __float_as_uint(r2) != __float_as_uint(ref);
    if (safe) {
      bad1 += m1; bad2 += m2;
      if (m1) { const unsigned long long slot = atomicAdd(&out[4], 1ull); if (slot < 56) out[8 + slot] = bits; }
    } else { obad1 += m1; obad2 += m2; }
  }
  if (bad1) atomicAdd(&out[0], bad1);
  if (bad2) atomicAdd(&out[1], bad2);
  if (obad1) atomicAdd(&out[2], obad1);
  if (obad2) atomicAdd(&out[3], obad2);
}
// normalize3's building blocks (rt_math.h): (a) the refined v_rsq_f32 against sqrtf for every FP32 pattern; (b) the quotient
// from the shared exact reciprocal against a / b for every significand of a and every `stride`-th significand of b (a, b in
// [1, 2): exponents do not matter while nothing under- or overflows).  out[0] = mismatches of (a) for 2^-60 <= x <= 2^60,
// out[1] = mismatches of (b), out[2] = pairs checked by (b), out[3] = a mismatching pattern of (a), out[4] = one of (b).
__global__ __launch_bounds__(256) void k_selftest_sqrt(unsigned long long* out) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  unsigned long long bad = 0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
    const uint32_t bits = (uint32_t)i;
    if (bits < 0x21800000u || bits > 0x5d800000u) continue;              // 2^-60 .. 2^60
    const float x = __uint_as_float(bits);
    const float y = __builtin_amdgcn_rsqf(x);
    const float s = x * y, h = 0.5f * y;
    const float len = __builtin_fmaf(__builtin_fmaf(-s, s, x), h, s);
    if (__float_as_uint(len) != __float_as_uint(sqrtf(x))) { ++bad; out[3] = bits; }
  }
  if (bad) atomicAdd(&out[0], bad);
}
__global__ __launch_bounds__(256) void k_selftest_div(unsigned long long* out, unsigned int stride, unsigned int count) {
  const unsigned int t = blockIdx.x * 256u + threadIdx.x;
  if (t >= count) return;
  const unsigned int mb = t * stride;
  const float b = __uint_as_float(0x3f800000u | mb);
  const float r = rcp_newton(b, 1);
  unsigned long long bad = 0;
  for (unsigned int ma = 0; ma < (1u << 23); ++ma) {
    const float a = __uint_as_float(0x3f800000u | ma);
    const float q0 = a * r;
    const float q = __builtin_fmaf(__builtin_fmaf(-b, q0, a), r, q0);
    if (__float_as_uint(q) != __float_as_uint(a / b)) { ++bad; out[4] = ((unsigned long long)ma << 32) | mb; }
  }
  if (bad) atomicAdd(&out[1], bad);
}
// shade() (rt_wave_common.h) on caller-given lanes: one wave per block, the wave's sample count from ns[].  SL: the
// instantiation specialised on the sample count where there is a case for it below.
template <int SS>
__device__ __forceinline__ f3 selftest_shade_one(bool lit, bool secondary, int unshadowed, int NS, float term, float4 col) {
  const float inv_S = (NS & (NS - 1)) == 0 ? 1.0f / (float)NS : 0.0f;           // as the host fills FrameParams::inv_S
  return shade<SS>(lit, secondary, unshadowed, NS, term, inv_S, col, shade_sum_needed(lit, term));
}
template <bool SL>
__global__ __launch_bounds__(64) void k_selftest_shade(const int* __restrict__ ns, const int* __restrict__ lit,
                                                       const int* __restrict__ secondary, const int* __restrict__ unshadowed,
                                                       const float* __restrict__ term, const float4* __restrict__ col,
                                                       float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  const int NS = __builtin_amdgcn_readfirstlane(ns[blockIdx.x]);
  const bool l = lit[i] != 0, sec = secondary[i] != 0;
  const int u = unshadowed[i];
  const float t = term[i];
  const float4 c = col[i];
  f3 r;
  if (SL && NS == 1) r = selftest_shade_one<1>(l, sec, u, 1, t, c);
  else if (SL && NS == 5) r = selftest_shade_one<5>(l, sec, u, 5, t, c);
  else if (SL && NS == 10) r = selftest_shade_one<10>(l, sec, u, 10, t, c);
  else if (SL && NS == 16) r = selftest_shade_one<16>(l, sec, u, 16, t, c);
  else if (SL && NS == 64) r = selftest_shade_one<64>(l, sec, u, 64, t, c);
  else r = selftest_shade_one<0>(l, sec, u, NS, t, c);
  out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
}
// all_within() (rt_wave_common.h) beside the reduction it stands for, one wave per block with the wave's bound from bound[]:
// out[2 w] = all_within, out[2 w + 1] = wave_max_pos(in ? v : 0.0f) <= bound.
__global__ __launch_bounds__(64) void k_selftest_all_within(const int* __restrict__ in, const float* __restrict__ v,
                                                            const float* __restrict__ bound, int* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  const float b = uniform(bound[blockIdx.x]);
  const bool lane_in = in[i] != 0;
  const float x = v[i];
  const bool got = all_within(ballot(lane_in), x, b);
  const bool want = wave_max_pos(lane_in ? x : 0.0f) <= b;
  if (threadIdx.x == 0) { out[2 * blockIdx.x] = got ? 1 : 0; out[2 * blockIdx.x + 1] = want ? 1 : 0; }
}
}  // namespace uobrt

extern "C" int rt_selftest_all_within(int32_t nwaves, const int32_t* in, const float* v, const float* bound, int32_t* out) {
  using namespace uobrt;
  if (nwaves < 1 || nwaves > (1 << 20) || !in || !v || !bound || !out) {
    set_error("rt_selftest_all_within: NULL argument or wave count outside 1 .. 2^20"); return RT_E_INVALID;
  }
  const size_t n = (size_t)nwaves * 64;
  DevMem<int> d_int;                  // in, out
  DevMem<float> d_f;                  // v, bound
  if (d_int.alloc(n + 2 * (size_t)nwaves) != hipSuccess || d_f.alloc(n + (size_t)nwaves) != hipSuccess) {
    set_error("hipMalloc failed (no device?)"); return RT_E_DEVICE;
  }
  hipError_t e = hipMemcpy(d_int.p, in, n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_f.p, v, n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_f.p + n, bound, (size_t)nwaves * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { set_error("rt_selftest_all_within: %s", hipGetErrorString(e)); return RT_E_DEVICE; }
  hipLaunchKernelGGL(k_selftest_all_within, dim3(nwaves), dim3(64), 0, 0, d_int.p, d_f.p, d_f.p + n, d_int.p + n);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(out, d_int.p + n, (size_t)nwaves * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { set_error("rt_selftest_all_within: %s", hipGetErrorString(e)); return RT_E_DEVICE; }
  return RT_OK;
}

extern "C" int rt_selftest_shade(int32_t nwaves, const int32_t* ns, const int32_t* lit, const int32_t* secondary,
                                 const int32_t* unshadowed, const float* term, const float* col, int32_t straight_line, float* out) {
  using namespace uobrt;
  if (nwaves < 1 || nwaves > (1 << 20) || !ns || !lit || !secondary || !unshadowed || !term || !col || !out) {
    set_error("rt_selftest_shade: NULL argument or wave count outside 1 .. 2^20"); return RT_E_INVALID;
  }
  for (int w = 0; w < nwaves; ++w)
    if (ns[w] < 1 || ns[w] > 4096) { set_error("rt_selftest_shade: ns[%d] = %d outside 1 .. 4096", w, ns[w]); return RT_E_INVALID; }
  const size_t n = (size_t)nwaves * 64;
  DevMem<int> d_ns, d_int;            // d_int: lit, secondary, unshadowed
  DevMem<float> d_f;                  // term, col, out
  if (d_ns.alloc((size_t)nwaves) != hipSuccess || d_int.alloc(3 * n) != hipSuccess || d_f.alloc(8 * n) != hipSuccess) {
    set_error("hipMalloc failed (no device?)"); return RT_E_DEVICE;
  }
  hipError_t e = hipMemcpy(d_ns.p, ns, (size_t)nwaves * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_int.p, lit, n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_int.p + n, secondary, n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_int.p + 2 * n, unshadowed, n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_f.p, term, n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_f.p + n, col, n * 16, hipMemcpyHostToDevice);
  if (e != hipSuccess) { set_error("rt_selftest_shade: %s", hipGetErrorString(e)); return RT_E_DEVICE; }
  const float4* d_col = reinterpret_cast<const float4*>(d_f.p + n);
  if (straight_line)
    hipLaunchKernelGGL(k_selftest_shade<true>, dim3(nwaves), dim3(64), 0, 0, d_ns.p, d_int.p, d_int.p + n, d_int.p + 2 * n, d_f.p, d_col, d_f.p + 5 * n);
  else
    hipLaunchKernelGGL(k_selftest_shade<false>, dim3(nwaves), dim3(64), 0, 0, d_ns.p, d_int.p, d_int.p + n, d_int.p + 2 * n, d_f.p, d_col, d_f.p + 5 * n);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(out, d_f.p + 5 * n, n * 12, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { set_error("rt_selftest_shade: %s", hipGetErrorString(e)); return RT_E_DEVICE; }
  return RT_OK;
}

extern "C" int rt_selftest_normalize(uint64_t out[8], uint32_t b_stride) {
  using namespace uobrt;
  if (!out || b_stride == 0 || b_stride > (1u << 23)) { set_error("rt_selftest_normalize: NULL argument or stride outside 1 .. 2^23"); return RT_E_INVALID; }
  DevMem<unsigned long long> d;
  if (d.alloc(8) != hipSuccess) { set_error("hipMalloc failed (no device?)"); return RT_E_DEVICE; }
  hipMemset(d, 0, 8 * 8);
  const unsigned int count = ((1u << 23) + b_stride - 1) / b_stride;
  hipLaunchKernelGGL(k_selftest_sqrt, dim3(16384), dim3(256), 0, 0, d.p);
  hipLaunchKernelGGL(k_selftest_div, dim3((count + 255) / 256), dim3(256), 0, 0, d.p, b_stride, count);
  const hipError_t e = hipMemcpy(out, d, 8 * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { set_error("rt_selftest_normalize: %s", hipGetErrorString(e)); return RT_E_DEVICE; }
  out[2] = (uint64_t)count << 23;
  return RT_OK;
}

extern "C" int rt_selftest_rcp(uint64_t out[64]) {
  using namespace uobrt;
  if (!out) { set_error("NULL argument"); return RT_E_INVALID; }
  DevMem<unsigned long long> d;
  if (d.alloc(64) != hipSuccess) { set_error("hipMalloc failed (no device?)"); return RT_E_DEVICE; }
  hipMemset(d, 0, 64 * 8);
  hipLaunchKernelGGL(k_selftest_rcp, dim3(16384), dim3(256), 0, 0, d.p);
  const hipError_t e = hipMemcpy(out, d, 64 * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { set_error("rt_selftest_rcp: %s", hipGetErrorString(e)); return RT_E_DEVICE; }
  return RT_OK;
}
