// rt_scene_pose.hip — the device half of rt_pose_objects / rt_pose_objects_device (include/uob_rt.h "rigid objects") and of
// rt_pose_skin / rt_pose_skin_device ("skinned meshes").
//
// Two kernels over the rest pose (vertices and normals as rt_set_objects / rt_set_skin snapshot them), one lane per triangle:
// rt_pose_triangles takes one xform12 per object, rt_skin_triangles one xform12 per bone and four (bone, weight) influences
// per corner of the skinned range.  Both write the posed vertices and normals into the staging scene the context owns.  From
// there the posed scene takes rt_update_scene_device's path (rt_scene_check, then the copy into the live buffers, then
// rt_scene_refit or the tile build), so a pose that fails the check has touched nothing a frame reads.
//
// The arithmetic is rt_scene_transform's and rt_scene_skin's (scene.cpp), operation for operation: this file is built with
// -ffp-contract=off, and '/' and sqrtf are correctly rounded at the project's flags (rt_math.h), denormal operands and results
// included.  The one place where the two sides could differ is the NaN of a degenerate triangle, 0 * (1 / sqrt(0)): an x86
// host writes the default NaN with the sign bit set, so the kernels write that pattern for any NaN component.  (In a scene
// that passes the check no other NaN can arise: the edges stay within 2^17 and the squared length of the cross product below
// 2^72.  A NaN vertex, the 0 * inf of a blend included, fails the check whatever its bits.)
#include <hip/hip_runtime.h>

#include "rt_host.h"

namespace uobrt {

__device__ inline float3 pose_point(const float4 v, const float* __restrict__ m) {
  float3 r;
  r.x = ((v.x * m[0] + v.y * m[1]) + v.z * m[2]) + m[3];
  r.y = ((v.x * m[4] + v.y * m[5]) + v.z * m[6]) + m[7];
  r.z = ((v.x * m[8] + v.y * m[9]) + v.z * m[10]) + m[11];
  return r;
}

__device__ inline float host_nan(float x) { return x != x ? __uint_as_float(0xffc00000u) : x; }

// rt_triangle_compute_normal: cross(e2, e1) * (1 / sqrt(dot)), the dot summed left to right
__device__ inline float4 pose_normal(const float3 p0, const float3 p1, const float3 p2) {
  const float e1x = p1.x - p0.x, e1y = p1.y - p0.y, e1z = p1.z - p0.z;
  const float e2x = p2.x - p0.x, e2y = p2.y - p0.y, e2z = p2.z - p0.z;
  const float nx = e2y * e1z - e1y * e2z;
  const float ny = e2z * e1x - e1z * e2x;
  const float nz = e2x * e1y - e1x * e2y;
  const float inv = 1.0f / sqrtf(nx * nx + ny * ny + nz * nz);
  return make_float4(host_nan(nx * inv), host_nan(ny * inv), host_nan(nz * inv), 0.0f);   // (w = 0: rt_scene_pack's)
}

// One lane per triangle, grid-stride.  object_of[i] = the object of triangle i, kPoseStatic = in no object.
__global__ __launch_bounds__(256) void rt_pose_triangles(const float4* __restrict__ rest_v, const float4* __restrict__ rest_n,
                                                         const unsigned short* __restrict__ object_of,
                                                         const float* __restrict__ xforms12, int n, float4* __restrict__ out_v,
                                                         float4* __restrict__ out_n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 a = rest_v[3 * (size_t)i], b = rest_v[3 * (size_t)i + 1], c = rest_v[3 * (size_t)i + 2];
    const unsigned int obj = object_of[i];
    if (obj == kPoseStatic) {
      out_v[3 * (size_t)i] = a; out_v[3 * (size_t)i + 1] = b; out_v[3 * (size_t)i + 2] = c;
      out_n[i] = rest_n[i];
      continue;
    }
    const float* const m = xforms12 + 12 * (size_t)obj;
    const float3 p0 = pose_point(a, m), p1 = pose_point(b, m), p2 = pose_point(c, m);
    out_v[3 * (size_t)i] = make_float4(p0.x, p0.y, p0.z, a.w);
    out_v[3 * (size_t)i + 1] = make_float4(p1.x, p1.y, p1.z, b.w);
    out_v[3 * (size_t)i + 2] = make_float4(p2.x, p2.y, p2.z, c.w);
    out_n[i] = pose_normal(p0, p1, p2);
  }
}

// rt_scene_skin's corner: the four rigid poses of v, blended left to right; every influence is evaluated, also at weight 0
__device__ inline float3 skin_point(const float4 v, const ushort4 j, const float4 w, const float* __restrict__ bones12) {
  const float3 p0 = pose_point(v, bones12 + 12 * (size_t)j.x), p1 = pose_point(v, bones12 + 12 * (size_t)j.y);
  const float3 p2 = pose_point(v, bones12 + 12 * (size_t)j.z), p3 = pose_point(v, bones12 + 12 * (size_t)j.w);
  float3 r;
  r.x = ((w.x * p0.x + w.y * p1.x) + w.z * p2.x) + w.w * p3.x;
  r.y = ((w.x * p0.y + w.y * p1.y) + w.z * p2.y) + w.w * p3.y;
  r.z = ((w.x * p0.z + w.y * p1.z) + w.z * p2.z) + w.w * p3.z;
  return r;
}

// One lane per triangle, grid-stride.  index / weights: one row per corner of the triangles [first, first + count), corner
// 0, 1, 2 of triangle first, then of first + 1, ...; a triangle outside the range is copied through.  The bones are read
// through the cache (why not through LDS).
__global__ __launch_bounds__(256) void rt_skin_triangles(const float4* __restrict__ rest_v, const float4* __restrict__ rest_n,
                                                         const ushort4* __restrict__ index, const float4* __restrict__ weights,
                                                         const float* __restrict__ bones12, int n, int first, int count,
                                                         float4* __restrict__ out_v, float4* __restrict__ out_n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 a = rest_v[3 * (size_t)i], b = rest_v[3 * (size_t)i + 1], c = rest_v[3 * (size_t)i + 2];
    if (i < first || i - first >= count) {
      out_v[3 * (size_t)i] = a; out_v[3 * (size_t)i + 1] = b; out_v[3 * (size_t)i + 2] = c;
      out_n[i] = rest_n[i];
      continue;
    }
    const size_t k = 3 * (size_t)(i - first);
    const float3 p0 = skin_point(a, index[k], weights[k], bones12);
    const float3 p1 = skin_point(b, index[k + 1], weights[k + 1], bones12);
    const float3 p2 = skin_point(c, index[k + 2], weights[k + 2], bones12);
    out_v[3 * (size_t)i] = make_float4(p0.x, p0.y, p0.z, a.w);
    out_v[3 * (size_t)i + 1] = make_float4(p1.x, p1.y, p1.z, b.w);
    out_v[3 * (size_t)i + 2] = make_float4(p2.x, p2.y, p2.z, c.w);
    out_n[i] = pose_normal(p0, p1, p2);
  }
}

// Both kernels: at most 2048 workgroups of 256 lanes, which stride over larger scenes
static int pose_blocks(int n) { return n > 2048 * 256 ? 2048 : (n + 255) / 256; }

void launch_pose(const float4* rest_v, const float4* rest_n, const unsigned short* object_of, const float* d_xforms12, int n,
                 float4* out_v, float4* out_n, hipStream_t stream) {
  if (n <= 0) return;
  rt_pose_triangles<<<pose_blocks(n), 256, 0, stream>>>(rest_v, rest_n, object_of, d_xforms12, n, out_v, out_n);
}

void launch_skin(const float4* rest_v, const float4* rest_n, const ushort4* index, const float4* weights, const float* d_bones12,
                 int n, int first, int count, float4* out_v, float4* out_n, hipStream_t stream) {
  if (n <= 0) return;
  rt_skin_triangles<<<pose_blocks(n), 256, 0, stream>>>(rest_v, rest_n, index, weights, d_bones12, n, first, count, out_v, out_n);
}

}  // namespace uobrt
