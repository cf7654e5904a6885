// motion_host.cpp — the motion planes of include/uob_rt.h ("rt_motion_planes"), stated once on the host: a plain loop that is
// the definition, line for line, and the argument checks that every entry applies.  Host only (no device, no context); built
// with -ffp-contract=off like everything else, so that every product, sum and quotient below is one FP32 operation.  The
// device kernel (rt_motion.hip) is pinned against this file bit for bit.
#include <cstdint>
#include <cstring>

#include "../../include/uob_rt.h"

namespace uobrt {
void set_error(const char* fmt, ...);

// The element planes and their count; fn names the entry in the message
int motion_check(const void* prim, const void* position4, const void* normal4, int64_t count, const void* out_prev_position4,
                 const void* out_prev_normal4, const char* fn) {
  if (!prim || !position4 || !normal4 || !out_prev_position4 || !out_prev_normal4) {
    set_error("%s: NULL plane (prim / position4 / normal4 / out_prev_position4 / out_prev_normal4)", fn); return RT_E_INVALID;
  }
  if (count < 0 || count > (int64_t(1) << 31)) { set_error("%s: count = %lld outside [0, 2^31]", fn, (long long)count); return RT_E_INVALID; }
  return RT_OK;
}
}  // namespace uobrt

namespace {

float quiet_if_nan(float v) {
  if (v != v) { const uint32_t quiet = 0x7FC00000u; memcpy(&v, &quiet, 4); }
  return v;
}

float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

}  // namespace

extern "C" {

int rt_motion_planes_host(const float* vertices4_now, const float* vertices4_then, const float* normals4_then, int32_t n,
                          const int32_t* prim, const float* position4, const float* normal4, int64_t count,
                          float* out_prev_position4, float* out_prev_normal4) {
  const int rc = uobrt::motion_check(prim, position4, normal4, count, out_prev_position4, out_prev_normal4, "rt_motion_planes_host");
  if (rc != RT_OK) return rc;
  if (n < 0) { uobrt::set_error("rt_motion_planes_host: n = %d below 0", n); return RT_E_INVALID; }
  if (n > 0 && (!vertices4_now || !vertices4_then || !normals4_then)) {
    uobrt::set_error("rt_motion_planes_host: NULL scene (vertices4_now / vertices4_then / normals4_then)"); return RT_E_INVALID;
  }
  for (int64_t k = 0; k < count; ++k) {
    const float* P = position4 + 4 * k;
    float* oP = out_prev_position4 + 4 * k;
    float* oN = out_prev_normal4 + 4 * k;
    const int32_t t = prim[k];
    if (!(P[3] > 0.0f) || t < -2 || t >= n) {              // no place in the previous scene
      memset(oP, 0, 16);
      memset(oN, 0, 16);
      continue;
    }
    const int64_t tri = t >= 0 ? t : 0;                    // (a miss or a sphere reads no triangle)
    const float* a = vertices4_now + 12 * tri;
    const float* b = a + 4;
    const float* c = a + 8;
    const float* a0 = vertices4_then + 12 * tri;
    const float* b0 = a0 + 4;
    const float* c0 = a0 + 8;
    bool moved = false;
    if (t >= 0)
      for (int j = 0; j < 3; ++j) moved = moved || !(a[j] == a0[j]) || !(b[j] == b0[j]) || !(c[j] == c0[j]);
    if (!moved) {                                          // a miss, a sphere, an unmoved triangle: the planes' own bits
      memcpy(oP, P, 16);
      memcpy(oN, normal4 + 4 * k, 16);
      continue;
    }
    float e1[3], e2[3], d[3], f1[3], f2[3];
    for (int j = 0; j < 3; ++j) {
      e1[j] = b[j] - a[j];
      e2[j] = c[j] - a[j];
      d[j] = P[j] - a[j];
      f1[j] = b0[j] - a0[j];
      f2[j] = c0[j] - a0[j];
    }
    const float d11 = dot3(e1, e1), d12 = dot3(e1, e2), d22 = dot3(e2, e2), p1 = dot3(d, e1), p2 = dot3(d, e2);
    const float den = d11 * d22 - d12 * d12;
    const float u = (d22 * p1 - d12 * p2) / den;
    const float v = (d11 * p2 - d12 * p1) / den;
    for (int j = 0; j < 3; ++j) oP[j] = quiet_if_nan((a0[j] + u * f1[j]) + v * f2[j]);
    oP[3] = 1.0f;
    memcpy(oN, normals4_then + 4 * (int64_t)t, 12);
    oN[3] = 0.0f;
  }
  return RT_OK;
}

}  // extern "C"
