// accumulate_host.cpp — the temporal reprojection of include/uob_rt.h ("rt_accumulate_plane", and "rt_accumulate_plane_moving"
// with its reprojection planes), stated once on the host: a plain loop nest that is the definition, line for line, and the
// checks of rt_accumulate_params that every entry applies.
// Host only (no device, no context); built with -ffp-contract=off like everything else, so that every product and sum below
// is one FP32 operation.  The device kernel (rt_accumulate.hip) is pinned against this file bit for bit.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/uob_rt.h"

namespace uobrt {
void set_error(const char* fmt, ...);

// The ranges of rt_accumulate_params and the plane pointers; fn names the entry in the message
int accumulate_check(const rt_accumulate_params* p, const void* value, const void* position4, const void* normal4, const void* prev,
                     const void* next, const char* fn) {
  if (!p) { set_error("%s: params is NULL", fn); return RT_E_INVALID; }
  if (!value || !position4 || !normal4 || !next) { set_error("%s: NULL plane (value / position4 / normal4 / next)", fn); return RT_E_INVALID; }
  if (next == prev) { set_error("%s: next must not be the same pointer as prev", fn); return RT_E_INVALID; }
  if (p->width < 1) { set_error("%s: width = %d below 1", fn, p->width); return RT_E_INVALID; }
  if (p->height < 1) { set_error("%s: height = %d below 1", fn, p->height); return RT_E_INVALID; }
  if ((int64_t)p->width * p->height > (int64_t(1) << 31)) {
    set_error("%s: width * height = %lld beyond 2^31", fn, (long long)p->width * p->height); return RT_E_INVALID;
  }
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(p->prev_rot[k])) { set_error("%s: prev_rot[%d] is not finite", fn, k); return RT_E_INVALID; }
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(p->prev_cam[k])) { set_error("%s: prev_cam[%d] is not finite", fn, k); return RT_E_INVALID; }
  if (!(p->prev_focal_px > 0.0f) || !std::isfinite(p->prev_focal_px)) {
    set_error("%s: prev_focal_px must be finite and > 0", fn); return RT_E_INVALID;
  }
  if (std::isnan(p->normal_min_dot)) { set_error("%s: normal_min_dot is NaN", fn); return RT_E_INVALID; }
  if (!(p->plane_eps >= 0.0f)) { set_error("%s: plane_eps must be >= 0 and not NaN", fn); return RT_E_INVALID; }
  if (p->max_history < 1 || p->max_history > 65536) {
    set_error("%s: max_history = %d outside [1, 65536]", fn, p->max_history); return RT_E_INVALID;
  }
  return RT_OK;
}

// The reprojection planes of rt_accumulate_plane_moving: both or neither
int accumulate_reproj_check(const void* reproj_position4, const void* reproj_normal4, const char* fn) {
  if ((reproj_position4 == nullptr) != (reproj_normal4 == nullptr)) {
    set_error("%s: reproj_position4 and reproj_normal4 must both be given or both be NULL", fn); return RT_E_INVALID;
  }
  return RT_OK;
}
}  // namespace uobrt

namespace {

float quiet_if_nan(float v) {
  if (v != v) { const uint32_t quiet = 0x7FC00000u; memcpy(&v, &quiet, 4); }
  return v;
}

// The definition over a plane; rpos / rnrm: the reprojection planes of rt_accumulate_plane_moving, or both NULL
int accumulate_planes(const rt_accumulate_params* p, const float* value, const float* position4, const float* normal4,
                      const int32_t* prim, const float* rpos, const float* rnrm, const rt_history_texel* prev, rt_history_texel* next,
                      float* out_mean, float* out_variance, const char* fn) {
  int rc = uobrt::accumulate_check(p, value, position4, normal4, prev, next, fn);
  if (rc == RT_OK) rc = uobrt::accumulate_reproj_check(rpos, rnrm, fn);
  if (rc != RT_OK) return rc;
  const int64_t w = p->width, h = p->height;
  const float* rot = p->prev_rot;
  const float half_w = 0.5f * (float)p->width, half_h = 0.5f * (float)p->height;
  const float nmax = (float)(p->max_history - 1);
  for (int64_t y = 0; y < h; ++y)
    for (int64_t x = 0; x < w; ++x) {
      const int64_t c = y * w + x;
      const float* P = position4 + 4 * c;
      const float* N = normal4 + 4 * c;
      const float* Pr = rpos ? rpos + 4 * c : P;         // what is projected and tested against the records
      const float* Nr = rpos ? rnrm + 4 * c : N;
      const float v = value[c];
      const float vv = v * v;
      const bool valid = P[3] > 0.0f;
      float num = 0.0f, num2 = 0.0f, den = 0.0f, cmin = INFINITY;
      int taps = 0;
      if (valid && prev && Pr[3] > 0.0f) {
        const float d0 = Pr[0] - p->prev_cam[0], d1 = Pr[1] - p->prev_cam[1], d2 = Pr[2] - p->prev_cam[2];
        const float q0 = (d0 * rot[0] + d1 * rot[4]) + d2 * rot[8];
        const float q1 = (d0 * rot[1] + d1 * rot[5]) + d2 * rot[9];
        const float q2 = (d0 * rot[2] + d1 * rot[6]) + d2 * rot[10];
        const float fx = (q0 * p->prev_focal_px) / q2 + half_w;
        const float fy = (q1 * p->prev_focal_px) / q2 + half_h;
        if (q2 > 0.0f && fx >= -1.0f && fx < (float)p->width && fy >= -1.0f && fy < (float)p->height) {
          const float xf = floorf(fx), yf = floorf(fy);
          const float ax = fx - xf, ay = fy - yf;
          const int64_t x0 = (int64_t)xf, y0 = (int64_t)yf;
          for (int j = 0; j < 2; ++j)
            for (int i = 0; i < 2; ++i) {
              const int64_t qx = x0 + i, qy = y0 + j;
              if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
              const float wt = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
              if (!(wt > 0.0f)) continue;
              const rt_history_texel& r = prev[qy * w + qx];
              if (!(r.count > 0.0f)) continue;
              if (prim && r.prim != prim[c]) continue;
              const float nd = (Nr[0] * r.normal[0] + Nr[1] * r.normal[1]) + Nr[2] * r.normal[2];
              if (!(nd >= p->normal_min_dot)) continue;
              const float e0 = r.position[0] - Pr[0], e1 = r.position[1] - Pr[1], e2 = r.position[2] - Pr[2];
              const float pd = (Nr[0] * e0 + Nr[1] * e1) + Nr[2] * e2;
              if (!(fabsf(pd) <= p->plane_eps)) continue;
              num = num + wt * r.mean;
              num2 = num2 + wt * r.m2;
              den = den + wt;
              if (r.count < cmin) cmin = r.count;
              ++taps;
            }
        }
      }
      rt_history_texel& o = next[c];
      memcpy(o.position, P, 12);
      memcpy(o.normal, N, 12);
      float mean, m2;
      if (taps == 0) {
        memcpy(&o.mean, &value[c], 4);             // the value's own bits
        memcpy(&mean, &value[c], 4);
        m2 = quiet_if_nan(vv);
        o.count = valid ? 1.0f : 0.0f;
      } else {
        const float mp = num / den, sp = num2 / den;
        const float n = (cmin < nmax ? cmin : nmax) + 1.0f;
        const float a = 1.0f / n;
        const float t1 = v - mp;
        mean = quiet_if_nan(mp + a * t1);
        const float t2 = vv - sp;
        m2 = quiet_if_nan(sp + a * t2);
        o.mean = mean;
        o.count = n;
      }
      o.m2 = m2;
      o.prim = prim ? prim[c] : -1;
      o.pad[0] = o.pad[1] = 0.0f;
      if (out_mean) memcpy(&out_mean[c], &o.mean, 4);
      if (out_variance) {
        const float t = m2 - mean * mean;
        out_variance[c] = t > 0.0f ? t : 0.0f;
      }
    }
  return RT_OK;
}

}  // namespace

extern "C" {

void rt_accumulate_params_default(rt_accumulate_params* p, int32_t width, int32_t height) {
  if (!p) return;
  p->width = width;
  p->height = height;
  for (int k = 0; k < 12; ++k) p->prev_rot[k] = (k == 0 || k == 5 || k == 10) ? 1.0f : 0.0f;
  p->prev_cam[0] = p->prev_cam[1] = p->prev_cam[2] = 0.0f;
  p->prev_focal_px = (float)width;
  p->normal_min_dot = 0.9f;
  p->plane_eps = 0.01f;
  p->max_history = 32;
}

int rt_accumulate_plane_host(const rt_accumulate_params* p, const float* value, const float* position4, const float* normal4,
                             const int32_t* prim, const rt_history_texel* prev, rt_history_texel* next, float* out_mean,
                             float* out_variance) {
  return accumulate_planes(p, value, position4, normal4, prim, nullptr, nullptr, prev, next, out_mean, out_variance,
                           "rt_accumulate_plane_host");
}

int rt_accumulate_plane_moving_host(const rt_accumulate_params* p, const float* value, const float* position4, const float* normal4,
                                    const int32_t* prim, const float* reproj_position4, const float* reproj_normal4,
                                    const rt_history_texel* prev, rt_history_texel* next, float* out_mean, float* out_variance) {
  return accumulate_planes(p, value, position4, normal4, prim, reproj_position4, reproj_normal4, prev, next, out_mean, out_variance,
                           "rt_accumulate_plane_moving_host");
}

}  // extern "C"
