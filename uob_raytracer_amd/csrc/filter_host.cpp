// filter_host.cpp — the edge-stopping a-trous filter of include/uob_rt.h ("rt_filter_plane"), stated once on the host: a plain
// loop nest that is the definition, line for line, and the checks of rt_filter_params that every entry applies.  Host only
// (no device, no context); built with -ffp-contract=off like everything else, so that every product and sum below is one
// FP32 operation.  The device kernels (rt_filter.hip) are pinned against this file bit for bit.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/uob_rt.h"

namespace uobrt {
void set_error(const char* fmt, ...);

// The ranges of rt_filter_params and the plane pointers; fn names the entry in the message
int filter_check(const rt_filter_params* p, const void* value, const void* position4, const void* normal4, const void* out,
                 const char* fn) {
  if (!p) { set_error("%s: params is NULL", fn); return RT_E_INVALID; }
  if (!value || !position4 || !normal4 || !out) { set_error("%s: NULL plane (value / position4 / normal4 / out)", fn); return RT_E_INVALID; }
  if (p->width < 1) { set_error("%s: width = %d below 1", fn, p->width); return RT_E_INVALID; }
  if (p->height < 1) { set_error("%s: height = %d below 1", fn, p->height); return RT_E_INVALID; }
  if ((int64_t)p->width * p->height > (int64_t(1) << 31)) {
    set_error("%s: width * height = %lld beyond 2^31", fn, (long long)p->width * p->height); return RT_E_INVALID;
  }
  if (p->passes < 1 || p->passes > 8) { set_error("%s: passes = %d outside [1, 8]", fn, p->passes); return RT_E_INVALID; }
  if (std::isnan(p->normal_min_dot)) { set_error("%s: normal_min_dot is NaN", fn); return RT_E_INVALID; }
  if (!(p->plane_eps >= 0.0f)) { set_error("%s: plane_eps must be >= 0 and not NaN", fn); return RT_E_INVALID; }
  if (!(p->value_max_diff >= 0.0f)) { set_error("%s: value_max_diff must be >= 0 or +INFINITY, not NaN", fn); return RT_E_INVALID; }
  return RT_OK;
}
}  // namespace uobrt

namespace {

const float kTap[3] = {0.375f, 0.25f, 0.0625f};   // h[|d|]: 3/8, 1/4, 1/16

// One pass at tap spacing s with the value bound vmax (already scaled by 2^-i): src -> dst, which do not overlap
void filter_pass(const rt_filter_params& p, int s, float vmax, const float* src, const float* pos, const float* nrm, float* dst) {
  const int64_t w = p.width, h = p.height;
  for (int64_t y = 0; y < h; ++y)
    for (int64_t x = 0; x < w; ++x) {
      const int64_t c = y * w + x;
      const float vp = src[c];
      if (!(pos[4 * c + 3] > 0.0f)) { memcpy(&dst[c], &src[c], 4); continue; }
      const float* Pp = pos + 4 * c;
      const float* Np = nrm + 4 * c;
      float num = 0.0f, den = 0.0f;
      for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
          const int64_t qx = x + (int64_t)dx * s, qy = y + (int64_t)dy * s;
          const float wt = kTap[dx < 0 ? -dx : dx] * kTap[dy < 0 ? -dy : dy];
          float vq;
          if (dx == 0 && dy == 0) {
            vq = vp;
          } else {
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
            const int64_t q = qy * w + qx;
            if (!(pos[4 * q + 3] > 0.0f)) continue;
            const float* Pq = pos + 4 * q;
            const float* Nq = nrm + 4 * q;
            const float nd = (Np[0] * Nq[0] + Np[1] * Nq[1]) + Np[2] * Nq[2];
            if (!(nd >= p.normal_min_dot)) continue;
            const float d0 = Pq[0] - Pp[0], d1 = Pq[1] - Pp[1], d2 = Pq[2] - Pp[2];
            const float pd = (Np[0] * d0 + Np[1] * d1) + Np[2] * d2;
            if (!(fabsf(pd) <= p.plane_eps)) continue;
            vq = src[q];
            if (!(fabsf(vq - vp) <= vmax)) continue;
          }
          num = num + wt * vq;
          den = den + wt;
        }
      if (den == 0.140625f) { memcpy(&dst[c], &src[c], 4); continue; }   // only the centre: the value's own bits
      float r = num / den;
      if (r != r) { const uint32_t quiet = 0x7FC00000u; memcpy(&r, &quiet, 4); }
      dst[c] = r;
    }
}

}  // namespace

extern "C" {

void rt_filter_params_default(rt_filter_params* p, int32_t width, int32_t height) {
  if (!p) return;
  p->width = width;
  p->height = height;
  p->passes = 5;
  p->normal_min_dot = 0.9f;
  p->plane_eps = 0.01f;
  p->value_max_diff = INFINITY;
}

int rt_filter_plane_host(const rt_filter_params* p, const float* value, const float* position4, const float* normal4, float* out) {
  const int rc = uobrt::filter_check(p, value, position4, normal4, out, "rt_filter_plane_host");
  if (rc != RT_OK) return rc;
  const size_t count = (size_t)p->width * p->height;
  std::vector<float> a(count), b(p->passes > 1 ? count : 0);   // no pass reads what it writes, also when out == value
  const float* src = value;
  for (int i = 0; i < p->passes; ++i) {
    float* dst = (i & 1) ? b.data() : a.data();
    const float vmax = p->value_max_diff * ldexpf(1.0f, -i);     // one product by an exact power of two; +INFINITY stays
    filter_pass(*p, 1 << i, vmax, src, position4, normal4, dst);
    src = dst;
  }
  memcpy(out, src, count * sizeof(float));
  return RT_OK;
}

}  // extern "C"
