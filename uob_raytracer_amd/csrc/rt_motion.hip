// rt_motion.hip — the motion planes of include/uob_rt.h ("rt_motion_planes") on the device, DESIGN.md 4.8c: where each
// element's surface point was in the scene the context's snapshot holds.  A call is one launch over the elements and a
// one-wave launch that sums the counters.  One lane per element: the three input planes are 16-byte loads (prim 4), the two
// triangles are gathered from the ORIGINAL-order arrays of the live scene and of the snapshot — neighbouring pixels share a
// triangle, so those loads hit the cache — and the two outputs are 16-byte stores.  host statement: motion_host.cpp.
#include "rt_host.h"

namespace uobrt {

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == 256, "flush_counters sums four waves");
enum { M_ELEMENTS = 0, M_VALID = 1, M_MOVED = 2, M_UNMOVED = 3, M_COPIED = 4, M_RANGE = 5 };
// Behind the exported counters: the accumulate kernel's scheme — kCounterSlots partial sums of (moved, unmoved, copied, out
// of range), one 128-byte line each, a workgroup adds to the slot of its index; the last launch of a call sums them
constexpr int kCounterSlots = 64, kSlotWords = 16, kSlotBase = 8, kCounters = 4;

struct MotionArgs {
  long count;
  int n;                           // triangles of the live scene and of the snapshot
  unsigned blocks_x;               // workgroups per grid.x; beyond that they continue in grid.y
  const int* prim;
  const float4* pos;
  const float4* nrm;
  const float4* v_now;
  const float4* v_then;
  const float4* n_then;
  float4* out_pos;
  float4* out_nrm;
};

__device__ __forceinline__ float quiet_if_nan(float v) { return v == v ? v : __uint_as_float(0x7FC00000u); }
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

__device__ __forceinline__ void flush_counters(unsigned long long* stats, bool moved, bool unmoved, bool copied, bool range) {
  __shared__ unsigned int s_count[kCounters][4];
  const unsigned int mine[kCounters] = {(unsigned int)__popcll(__ballot(moved)), (unsigned int)__popcll(__ballot(unmoved)),
                                        (unsigned int)__popcll(__ballot(copied)), (unsigned int)__popcll(__ballot(range))};
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < kCounters; ++k) s_count[k][wave] = mine[k];
  __syncthreads();
  if (threadIdx.x < kCounters) {
    const int k = threadIdx.x;
    const unsigned int total = (s_count[k][0] + s_count[k][1]) + (s_count[k][2] + s_count[k][3]);
    const unsigned int slot = (blockIdx.x + blockIdx.y * 7u) & (kCounterSlots - 1);
    if (total) atomicAdd(&stats[kSlotBase + slot * kSlotWords + k], (unsigned long long)total);
  }
}

__global__ __launch_bounds__(64) void rt_motion_counters(unsigned long long* stats, long count) {
  if (threadIdx.x != 0) return;
  unsigned long long sum[kCounters] = {0, 0, 0, 0};
  for (int s = 0; s < kCounterSlots; ++s)
    for (int k = 0; k < kCounters; ++k) sum[k] += stats[kSlotBase + s * kSlotWords + k];
  stats[M_ELEMENTS] = (unsigned long long)count;
  stats[M_VALID] = (sum[0] + sum[1]) + sum[2];
  stats[M_MOVED] = sum[0];
  stats[M_UNMOVED] = sum[1];
  stats[M_COPIED] = sum[2];
  stats[M_RANGE] = sum[3];
}

__global__ __launch_bounds__(kThreads) void rt_motion_elements(MotionArgs a, unsigned long long* stats) {
  const long k = ((long)blockIdx.y * a.blocks_x + blockIdx.x) * kThreads + threadIdx.x;
  bool moved = false, unmoved = false, copied = false, range = false;
  if (k < a.count) {                                     // (whole workgroups beyond the last element fall through to the flush)
    const float4 P = a.pos[k], N = a.nrm[k];
    const int t = a.prim[k];
    float4 oP = make_float4(0.0f, 0.0f, 0.0f, 0.0f), oN = oP;      // no place in the previous scene
    if (P.w > 0.0f) {
      if (t < -2 || t >= a.n) {
        range = true;
      } else if (t < 0) {                                // a miss or a sphere: the planes' own bits
        copied = true;
        oP = P; oN = N;
      } else {
        const float4* now = a.v_now + 3 * (long)t;
        const float4* then = a.v_then + 3 * (long)t;
        const float4 A = now[0], B = now[1], C = now[2];
        const float4 A0 = then[0], B0 = then[1], C0 = then[2];
        unmoved = A.x == A0.x && A.y == A0.y && A.z == A0.z && B.x == B0.x && B.y == B0.y && B.z == B0.z && C.x == C0.x &&
                  C.y == C0.y && C.z == C0.z;
        if (unmoved) {
          oP = P; oN = N;
        } else {
          moved = true;
          const float e1x = B.x - A.x, e1y = B.y - A.y, e1z = B.z - A.z;
          const float e2x = C.x - A.x, e2y = C.y - A.y, e2z = C.z - A.z;
          const float dx = P.x - A.x, dy = P.y - A.y, dz = P.z - A.z;
          const float f1x = B0.x - A0.x, f1y = B0.y - A0.y, f1z = B0.z - A0.z;
          const float f2x = C0.x - A0.x, f2y = C0.y - A0.y, f2z = C0.z - A0.z;
          const float d11 = dot3(e1x, e1y, e1z, e1x, e1y, e1z), d12 = dot3(e1x, e1y, e1z, e2x, e2y, e2z);
          const float d22 = dot3(e2x, e2y, e2z, e2x, e2y, e2z);
          const float p1 = dot3(dx, dy, dz, e1x, e1y, e1z), p2 = dot3(dx, dy, dz, e2x, e2y, e2z);
          const float den = d11 * d22 - d12 * d12;
          const float u = (d22 * p1 - d12 * p2) / den;   // correctly rounded (the compiler's IEEE division)
          const float v = (d11 * p2 - d12 * p1) / den;
          const float4 Nt = a.n_then[t];
          oP = make_float4(quiet_if_nan((A0.x + u * f1x) + v * f2x), quiet_if_nan((A0.y + u * f1y) + v * f2y),
                           quiet_if_nan((A0.z + u * f1z) + v * f2z), 1.0f);
          oN = make_float4(Nt.x, Nt.y, Nt.z, 0.0f);
        }
      }
    }
    a.out_pos[k] = oP;
    a.out_nrm[k] = oN;
  }
  flush_counters(stats, moved, unmoved, copied, range);
}

}  // namespace

int motion_stats_words() { return kSlotBase + kCounterSlots * kSlotWords; }

void launch_motion(const float4* d_v_now, const float4* d_v_then, const float4* d_n_then, int n, const int* d_prim, const float4* d_pos,
                   const float4* d_nrm, long count, float4* d_out_pos, float4* d_out_nrm, int blocks_x, unsigned long long* stats,
                   hipStream_t stream) {
  const long blocks = (count + kThreads - 1) / kThreads;
  const long bx = blocks_x >= 1 && blocks_x <= kMotionBlocksX ? blocks_x : kMotionBlocksX;
  const dim3 grid((unsigned)(blocks < bx ? blocks : bx), (unsigned)((blocks + bx - 1) / bx));
  const MotionArgs a{count, n, (unsigned)bx, d_prim, d_pos, d_nrm, d_v_now, d_v_then, d_n_then, d_out_pos, d_out_nrm};
  hipLaunchKernelGGL(rt_motion_elements, grid, dim3(kThreads), 0, stream, a, stats);
  hipLaunchKernelGGL(rt_motion_counters, dim3(1), dim3(64), 0, stream, stats, count);
}

}  // namespace uobrt
