// rt_tile_build.hip — the mesh kernel's tiled ORDER, built on the device (rt_replace_scene_device, RT_UPDATE_DEVICE_TILES).
//
// Input: the scene's vertices in original order (device memory) and the vertices' box that rt_scene_check has reduced.
// Output: orig[n], orig[j] = original index of the triangle at tiled position j — index for index what the host's
// tiled_order(v4, n, /*morton=*/true) returns (rt_tile_sort.hip).  rt_scene_refit then gathers the tiled copy and writes
// the tiles' 12 floats for that order; nothing here computes tile data.
//
//   rt_tile_keys     one lane per triangle: the host's key, in the host's FP32 operations (the library is built with
//                    -ffp-contract=off; the one division, 1023 / ext, is done by the host and passed in).  A "large"
//                    triangle (extent above a quarter of the scene's) gets key 0, the others 0x40000000 | morton(centre).
//   rt_sort_count /  LSD radix sort of (key, original index), 8 bits per pass, 4 passes (keys have 31 bits).  A chunk is
//   rt_sort_scan /   1024 consecutive elements, owned by ONE wave: count writes the chunk's 256 digit counts (digit-major
//   rt_sort_scatter  table), scan turns the table into start offsets (one workgroup, exclusive prefix sum), scatter walks the
//                    chunk again in order, 64 elements a round, and places every element behind the elements of its digit
//                    that come before it: lower chunks (the table), earlier rounds (a running count in LDS) and lower lanes
//                    of its round (ballots).  Every pass is therefore stable, so equal keys keep the order of their indices:
//                    the result is the unique sorted sequence of (key, index), which is what std::stable_sort leaves.
// Every store is an ordinary vector store; the scatter loop keeps no array in registers (no scratch).
#include <hip/hip_runtime.h>

#include "rt_host.h"

namespace uobrt {

constexpr int kSortRounds = 16;                    // rounds of 64 elements per chunk
constexpr int kSortChunk = 64 * kSortRounds;       // elements per chunk (one wave)
constexpr int kSortScanTile = 4096;                // table entries per step of the scan: 1024 lanes x 4

// 10 bits -> every third bit (rt_tile_sort.hip spread3)
__device__ inline unsigned int spread3_dev(unsigned int v) {
  v &= 1023u;
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

__global__ __launch_bounds__(256) void rt_tile_keys(const float4* __restrict__ v, int n, float lo0, float lo1, float lo2, float ext,
                                                    float inv, unsigned int* __restrict__ keys, int* __restrict__ idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p0 = v[3 * (size_t)i], p1 = v[3 * (size_t)i + 1], p2 = v[3 * (size_t)i + 2];
  const float a[3] = {p0.x, p0.y, p0.z}, b[3] = {p1.x, p1.y, p1.z}, c[3] = {p2.x, p2.y, p2.z}, lo[3] = {lo0, lo1, lo2};
  float tl[3], th[3];
  for (int k = 0; k < 3; ++k) { tl[k] = fminf(fminf(a[k], b[k]), c[k]); th[k] = fmaxf(fmaxf(a[k], b[k]), c[k]); }
  const float te = fmaxf(fmaxf(th[0] - tl[0], th[1] - tl[1]), th[2] - tl[2]);
  unsigned int code = 0u;
  if (!(te > 0.25f * ext)) {
    unsigned int q[3];
    for (int k = 0; k < 3; ++k) {
      const float f = (0.5f * (tl[k] + th[k]) - lo[k]) * inv;
      q[k] = f >= 0.0f ? (f < 1023.0f ? (unsigned int)f : 1023u) : 0u;
    }
    code = 0x40000000u | spread3_dev(q[0]) | (spread3_dev(q[1]) << 1) | (spread3_dev(q[2]) << 2);
  }
  keys[i] = code;
  idx[i] = i;
}

// table[d * nchunks + chunk] = number of elements of the chunk whose digit is d
__global__ __launch_bounds__(64) void rt_sort_count(const unsigned int* __restrict__ keys, int n, int shift, int nchunks,
                                                    unsigned int* __restrict__ table) {
  __shared__ unsigned int s_cnt[256];
  const int l = threadIdx.x, chunk = blockIdx.x;
  for (int d = l; d < 256; d += 64) s_cnt[d] = 0u;
  __syncthreads();
  const int base = chunk * kSortChunk;
  for (int r = 0; r < kSortRounds; ++r) {
    const int i = base + r * 64 + l;
    if (i < n) atomicAdd(&s_cnt[(keys[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  for (int d = l; d < 256; d += 64) table[(size_t)d * nchunks + chunk] = s_cnt[d];
}

// Exclusive prefix sum of table[total] in place; ONE workgroup of 1024 lanes, kSortScanTile entries a step
__global__ __launch_bounds__(1024) void rt_sort_scan(unsigned int* __restrict__ table, int total) {
  __shared__ unsigned int s_wave[16];
  __shared__ unsigned int s_step;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  unsigned int carry = 0u;
  for (int base = 0; base < total; base += kSortScanTile) {
    const int i0 = base + 4 * t;
    unsigned int x[4];
    for (int k = 0; k < 4; ++k) x[k] = i0 + k < total ? table[i0 + k] : 0u;
    const unsigned int own = x[0] + x[1] + x[2] + x[3];
    unsigned int incl = own;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned int y = __shfl_up(incl, o);
      if (lane >= o) incl += y;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (wave == 0) {
      const unsigned int w = lane < 16 ? s_wave[lane] : 0u;
      unsigned int wi = w;
      for (int o = 1; o < 16; o <<= 1) {
        const unsigned int y = __shfl_up(wi, o);
        if (lane >= o) wi += y;
      }
      if (lane < 16) s_wave[lane] = wi - w;
      if (lane == 15) s_step = wi;
    }
    __syncthreads();
    unsigned int run = carry + s_wave[wave] + (incl - own);
    for (int k = 0; k < 4; ++k) {
      if (i0 + k < total) table[i0 + k] = run;
      run += x[k];
    }
    carry += s_step;
    __syncthreads();                       // s_wave / s_step are rewritten by the next step
  }
}

__global__ __launch_bounds__(64) void rt_sort_scatter(const unsigned int* __restrict__ keys, const int* __restrict__ idx, int n,
                                                      int shift, int nchunks, const unsigned int* __restrict__ table,
                                                      unsigned int* __restrict__ keys_out, int* __restrict__ idx_out) {
  __shared__ unsigned int s_off[256];      // where the next element of each digit goes
  const int l = threadIdx.x, chunk = blockIdx.x;
  for (int d = l; d < 256; d += 64) s_off[d] = table[(size_t)d * nchunks + chunk];
  __syncthreads();
  const int base = chunk * kSortChunk;
  const unsigned long long below = (1ull << l) - 1ull;
  for (int r = 0; r < kSortRounds; ++r) {
    const int i = base + r * 64 + l;
    if (base + r * 64 >= n) break;         // (the same for the whole wave)
    const bool live = i < n;
    const unsigned int key = live ? keys[i] : 0u;
    const int src = live ? idx[i] : 0;
    const unsigned int d = (key >> shift) & 255u;
    unsigned long long same = __ballot(live);      // the live lanes of this round with the same digit
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long vote = __ballot(live && bit);
      same &= bit ? vote : ~vote;
    }
    const unsigned int rank = (unsigned int)__popcll(same & below);
    const unsigned int pos = live ? s_off[d] + rank : 0u;
    __syncthreads();
    if (live && rank == 0u) s_off[d] += (unsigned int)__popcll(same);
    __syncthreads();
    if (live && pos < (unsigned int)n) {   // (pos < n by construction; the test keeps a broken table from writing outside)
      keys_out[pos] = key;
      idx_out[pos] = src;
    }
  }
}

static int sort_chunks(int n) { return (n + kSortChunk - 1) / kSortChunk; }

// Device memory the build needs besides its output: two key and two index arrays, and the digit table
size_t tile_build_scratch_bytes(int n) {
  return ((size_t)4 * (size_t)n + (size_t)256 * (size_t)sort_chunks(n)) * sizeof(unsigned int);
}

// Enqueue the build for the n triangles of v (vertices' box lo..hi) on `stream`: orig[n] receives the order
int launch_tile_build(const float4* v, int n, const float lo[3], const float hi[3], int* orig, void* scratch, hipStream_t stream) {
  if (n <= 0) return 0;
  float ext = 0.0f;
  for (int k = 0; k < 3; ++k) ext = fmaxf(ext, hi[k] - lo[k]);
  const float inv = ext > 0.0f ? 1023.0f / ext : 0.0f;
  const int nchunks = sort_chunks(n);
  unsigned int* key_a = static_cast<unsigned int*>(scratch);
  unsigned int* key_b = key_a + n;
  int* idx_a = reinterpret_cast<int*>(key_b + n);
  int* idx_b = idx_a + n;
  unsigned int* table = reinterpret_cast<unsigned int*>(idx_b + n);
  rt_tile_keys<<<(n + 255) / 256, 256, 0, stream>>>(v, n, lo[0], lo[1], lo[2], ext, inv, key_a, idx_a);
  for (int pass = 0; pass < 4; ++pass) {
    const unsigned int* kin = (pass & 1) ? key_b : key_a;
    const int* iin = (pass & 1) ? idx_b : idx_a;
    unsigned int* kout = (pass & 1) ? key_a : key_b;
    int* iout = pass == 3 ? orig : ((pass & 1) ? idx_a : idx_b);
    rt_sort_count<<<nchunks, 64, 0, stream>>>(kin, n, 8 * pass, nchunks, table);
    rt_sort_scan<<<1, 1024, 0, stream>>>(table, 256 * nchunks);
    rt_sort_scatter<<<nchunks, 64, 0, stream>>>(kin, iin, n, 8 * pass, nchunks, table, kout, iout);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace uobrt
