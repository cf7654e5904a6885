// rt_scene_update.hip — the device half of rt_update_scene / rt_update_scene_device (include/uob_rt.h).
//
// Two kernels:
//   rt_scene_check  validates a scene in device memory (|x| <= 2^16, finite) and reduces what the host keeps of it:
//                   the non-glass triangle count (n_shadow) and the vertices' box.  Grid-stride loop, wave reductions,
//                   then one vector atomic per wave and word on a small result block (floats through order-preserving keys).
//   rt_scene_refit  keeps the tiling of rt_init (d_orig) and rebuilds the mesh kernel's copy of the scene for new vertices:
//                   one wave per 64-triangle tile gathers its triangles into the tiled arrays and computes the tile's 12
//                   floats with the same double operations, in the same order where order matters, as the host does
//                   for rt_init (rt_tile_sort.hip tile_data_host) — so a refit context renders what a new context renders.
#include <hip/hip_runtime.h>

#include "rt_host.h"

namespace uobrt {

// rt_scene_check's result block, in 32-bit words
enum { kCheckBad = 0, kCheckShadow = 1, kCheckLo = 2, kCheckHi = 5, kCheckWords = 8 };

// float -> unsigned key with the same order (negative floats: all bits flipped; positive: sign bit set)
__device__ inline unsigned int order_key(float f) {
  const unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void rt_scene_check(const float4* __restrict__ v, const float4* __restrict__ col, int n,
                                                      unsigned int* __restrict__ out) {
  unsigned int bad = 0u, shadow = 0u;
  unsigned int lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    for (int q = 0; q < 3; ++q) {
      const float4 p = v[3 * (size_t)i + q];
      const float x[3] = {p.x, p.y, p.z};
      for (int k = 0; k < 3; ++k) {
        bad += !(fabsf(x[k]) <= kMaxCoordinate);
        const unsigned int key = order_key(x[k]);
        lo[k] = min(lo[k], key);
        hi[k] = max(hi[k], key);
      }
    }
    shadow += col[i].w != -1.0f;
  }
  for (int o = 32; o > 0; o >>= 1) {
    bad += __shfl_xor(bad, o);
    shadow += __shfl_xor(shadow, o);
    for (int k = 0; k < 3; ++k) {
      lo[k] = min(lo[k], (unsigned int)__shfl_xor((int)lo[k], o));
      hi[k] = max(hi[k], (unsigned int)__shfl_xor((int)hi[k], o));
    }
  }
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicAdd(&out[kCheckBad], bad);
    if (shadow) atomicAdd(&out[kCheckShadow], shadow);
    for (int k = 0; k < 3; ++k) {
      atomicMin(&out[kCheckLo + k], lo[k]);
      atomicMax(&out[kCheckHi + k], hi[k]);
    }
  }
}

__device__ inline double wave_max(double x) {
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o));
  return x;
}

// One 64-lane workgroup per tile t: lane l takes tiled position j = 64 t + l (original triangle orig[j]).
__global__ __launch_bounds__(64) void rt_scene_refit(const float4* __restrict__ v, const float4* __restrict__ nrm,
                                                     const float4* __restrict__ col, const int* __restrict__ orig, int n,
                                                     float4* __restrict__ vm, float4* __restrict__ nm, float4* __restrict__ cm,
                                                     float4* __restrict__ tile_box) {
  __shared__ double s_q[64][3];
  __shared__ double s_ax[4];
  const int t = blockIdx.x, l = threadIdx.x;
  const int j0 = t * 64;
  const int cnt = min(64, n - j0);
  const bool live = l < cnt;
  float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  double q[3] = {0.0, 0.0, 0.0}, eta = 0.0, emax = 0.0;
  bool degenerate = false;
  if (live) {
    const int j = j0 + l, i = orig[j];
    const float4 p0 = v[3 * (size_t)i], p1 = v[3 * (size_t)i + 1], p2 = v[3 * (size_t)i + 2];
    vm[3 * (size_t)j] = p0; vm[3 * (size_t)j + 1] = p1; vm[3 * (size_t)j + 2] = p2;
    nm[j] = nrm[i];
    cm[j] = col[i];
    const float a[9] = {p0.x, p0.y, p0.z, p1.x, p1.y, p1.z, p2.x, p2.y, p2.z};
    for (int k = 0; k < 3; ++k) {
      lo[k] = fminf(fminf(fminf(lo[k], a[k]), a[3 + k]), a[6 + k]);
      hi[k] = fmaxf(fmaxf(fmaxf(hi[k], a[k]), a[3 + k]), a[6 + k]);
    }
    // the host's expressions term by term (built with -ffp-contract=off: no fused multiply-adds on either side)
    const double e1[3] = {(double)a[3] - a[0], (double)a[4] - a[1], (double)a[5] - a[2]};
    const double e2[3] = {(double)a[6] - a[0], (double)a[7] - a[1], (double)a[8] - a[2]};
    const double cr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double l1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]), l2 = sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
    const double lc = sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
    degenerate = !(lc > 1e-30) || !(l1 > 0) || !(l2 > 0) || !(lc >= 1e-9 * l1 * l2);
    if (!degenerate) {
      const double l3 = sqrt((e2[0] - e1[0]) * (e2[0] - e1[0]) + (e2[1] - e1[1]) * (e2[1] - e1[1]) + (e2[2] - e1[2]) * (e2[2] - e1[2]));
      const double le = fmax(fmax(l1, l2), l3);
      eta = le / lc;
      emax = le;
      for (int k = 0; k < 3; ++k) q[k] = cr[k] / lc;
    }
  }
  const bool any_degenerate = __ballot(degenerate) != 0ull;
  // every normal sign-aligned with the tile's first triangle's (lane 0 is always live)
  const double f0 = __shfl(q[0], 0), f1 = __shfl(q[1], 0), f2 = __shfl(q[2], 0);
  if (l > 0 && q[0] * f0 + q[1] * f1 + q[2] * f2 < 0) for (int k = 0; k < 3; ++k) q[k] = -q[k];
  for (int k = 0; k < 3; ++k) s_q[l][k] = q[k];
  __syncthreads();
  if (l == 0) {
    // the axis sum in triangle order, as the host adds it (a tree sum would round differently)
    double ax[3] = {0.0, 0.0, 0.0};
    for (int m = 0; m < cnt; ++m)
      for (int k = 0; k < 3; ++k) ax[k] += s_q[m][k];
    const double la = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    const bool cone = !any_degenerate && la > 1e-12;
    for (int k = 0; k < 3; ++k) s_ax[k] = cone ? ax[k] / la : (k == 0 ? 1.0 : 0.0);
    s_ax[3] = cone ? 1.0 : 0.0;
  }
  __syncthreads();
  const bool cone = s_ax[3] != 0.0;
  double chi = 0.0;
  if (live && cone) {
    const double dx = q[0] - s_ax[0], dy = q[1] - s_ax[1], dz = q[2] - s_ax[2];
    chi = sqrt(dx * dx + dy * dy + dz * dz);
  }
  chi = wave_max(chi);
  eta = wave_max(eta);
  emax = wave_max(emax);
  for (int o = 32; o > 0; o >>= 1)
    for (int k = 0; k < 3; ++k) {
      lo[k] = fminf(lo[k], __shfl_xor(lo[k], o));
      hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o));
    }
  if (!cone) { eta = 1e30; emax = 1e30; chi = 4.0; }
  if (l == 0) {
    tile_box[3 * (size_t)t] = make_float4(lo[0], lo[1], lo[2], (float)(eta * 1.0001));
    tile_box[3 * (size_t)t + 1] = make_float4(hi[0], hi[1], hi[2], (float)(emax * 1.0001));
    tile_box[3 * (size_t)t + 2] = make_float4((float)s_ax[0], (float)s_ax[1], (float)s_ax[2], (float)(chi * 1.0001 + 1e-6));
  }
}

// Enqueue the check of n triangles on `stream` into out[kCheckWords] (device memory, initialised here).
int launch_scene_check(const float4* v, const float4* col, int n, unsigned int* out, hipStream_t stream) {
  if (hipMemsetAsync(out, 0, kCheckWords * sizeof(unsigned int), stream) != hipSuccess ||
      hipMemsetAsync(out + kCheckLo, 0xff, 3 * sizeof(unsigned int), stream) != hipSuccess) return -1;
  if (n <= 0) return 0;
  int blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  rt_scene_check<<<blocks, 256, 0, stream>>>(v, col, n, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

void launch_scene_refit(const float4* v, const float4* nrm, const float4* col, const int* orig, int n, float4* vm, float4* nm,
                        float4* cm, float4* tile_box, hipStream_t stream) {
  if (n <= 0) return;
  rt_scene_refit<<<(n + 63) / 64, 64, 0, stream>>>(v, nrm, col, orig, n, vm, nm, cm, tile_box);
}

}  // namespace uobrt
