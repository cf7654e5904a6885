// filter_variance_host.cpp — the variance-guided a-trous filter of include/uob_rt.h ("rt_filter_plane_variance"), stated once
// on the host: a plain loop nest that is the definition, line for line, and the checks of rt_filter_variance_params that every
// entry applies.  Host only (no device, no context); built with -ffp-contract=off like everything else, so that every product
// and sum below is one FP32 operation.  The device kernels (rt_filter_variance.hip) are pinned against this file bit for bit.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/uob_rt.h"

namespace uobrt {
void set_error(const char* fmt, ...);
int filter_check(const rt_filter_params* p, const void* value, const void* position4, const void* normal4, const void* out,
                 const char* fn);

// The ranges of rt_filter_variance_params and the plane pointers (out_variance may be NULL); fn names the entry in the message
int filter_variance_check(const rt_filter_variance_params* p, const void* value, const void* variance, const void* position4,
                          const void* normal4, const void* out_value, const char* fn) {
  if (!p) { set_error("%s: params is NULL", fn); return RT_E_INVALID; }
  if (!value || !variance || !position4 || !normal4 || !out_value) {
    set_error("%s: NULL plane (value / variance / position4 / normal4 / out_value)", fn); return RT_E_INVALID;
  }
  const int rc = filter_check(&p->base, value, position4, normal4, out_value, fn);
  if (rc != RT_OK) return rc;
  if (!(p->sigma_value >= 0.0f)) { set_error("%s: sigma_value must be >= 0 or +INFINITY, not NaN", fn); return RT_E_INVALID; }
  if (!(p->value_eps >= 0.0f)) { set_error("%s: value_eps must be >= 0 or +INFINITY, not NaN", fn); return RT_E_INVALID; }
  return RT_OK;
}
}  // namespace uobrt

namespace {

const float kTap[3] = {0.375f, 0.25f, 0.0625f};   // h[|d|]: 3/8, 1/4, 1/16
const float kBlur[3] = {0.25f, 0.125f, 0.0625f};  // the threshold's 3 x 3 kernel by |dx| + |dy|

void store_bits(float* dst, uint32_t bits) { memcpy(dst, &bits, 4); }

// The value stop of one pass: T[p] = sigma * sqrt(3 x 3 blur of var at spacing 1) + eps for every valid pixel
void threshold_pass(const rt_filter_variance_params& vp, const float* var, const float* pos, float* T) {
  const int64_t w = vp.base.width, h = vp.base.height;
  for (int64_t y = 0; y < h; ++y)
    for (int64_t x = 0; x < w; ++x) {
      const int64_t c = y * w + x;
      if (!(pos[4 * c + 3] > 0.0f)) { T[c] = 0.0f; continue; }   // (never read: an invalid pixel takes no taps)
      float g = 0.0f;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int64_t qx = x + dx, qy = y + dy;
          const float k = kBlur[(dx != 0) + (dy != 0)];
          float cv = var[c];
          if (qx >= 0 && qx < w && qy >= 0 && qy < h && pos[4 * (qy * w + qx) + 3] > 0.0f) cv = var[qy * w + qx];
          g = g + k * cv;
        }
      T[c] = vp.sigma_value * sqrtf(g) + vp.value_eps;
    }
}

// One pass at tap spacing s with the value bound vmax (already scaled by 2^-i) and the thresholds T: (src, vsrc) -> (dst, vdst),
// which do not overlap
void filter_pass(const rt_filter_variance_params& vp, int s, float vmax, const float* T, const float* src, const float* vsrc,
                 const float* pos, const float* nrm, float* dst, float* vdst) {
  const rt_filter_params& p = vp.base;
  const int64_t w = p.width, h = p.height;
  for (int64_t y = 0; y < h; ++y)
    for (int64_t x = 0; x < w; ++x) {
      const int64_t c = y * w + x;
      const float vc = src[c];
      if (!(pos[4 * c + 3] > 0.0f)) { memcpy(&dst[c], &src[c], 4); memcpy(&vdst[c], &vsrc[c], 4); continue; }
      const float* Pp = pos + 4 * c;
      const float* Np = nrm + 4 * c;
      float num = 0.0f, den = 0.0f, num2 = 0.0f;
      for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
          const int64_t qx = x + (int64_t)dx * s, qy = y + (int64_t)dy * s;
          const float wt = kTap[dx < 0 ? -dx : dx] * kTap[dy < 0 ? -dy : dy];
          float vq, varq;
          if (dx == 0 && dy == 0) {
            vq = vc;
            varq = vsrc[c];
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
            const float dv = fabsf(vq - vc);
            if (!(dv <= vmax)) continue;
            if (!(dv <= T[c])) continue;
            varq = vsrc[q];
          }
          num = num + wt * vq;
          den = den + wt;
          num2 = num2 + (wt * wt) * varq;
        }
      if (den == 0.140625f) { memcpy(&dst[c], &src[c], 4); memcpy(&vdst[c], &vsrc[c], 4); continue; }   // only the centre: both planes' own bits
      const float r = num / den, r2 = num2 / (den * den);
      if (r != r) store_bits(&dst[c], 0x7FC00000u); else dst[c] = r;
      if (r2 != r2) store_bits(&vdst[c], 0x7FC00000u); else vdst[c] = r2;
    }
}

}  // namespace

extern "C" {

void rt_filter_variance_params_default(rt_filter_variance_params* p, int32_t width, int32_t height) {
  if (!p) return;
  rt_filter_params_default(&p->base, width, height);
  p->sigma_value = 4.0f;
  p->value_eps = 0.0f;
}

int rt_filter_plane_variance_host(const rt_filter_variance_params* p, const float* value, const float* variance, const float* position4,
                                  const float* normal4, float* out_value, float* out_variance) {
  const int rc = uobrt::filter_variance_check(p, value, variance, position4, normal4, out_value, "rt_filter_plane_variance_host");
  if (rc != RT_OK) return rc;
  const size_t count = (size_t)p->base.width * p->base.height;
  const int passes = p->base.passes;
  // no pass reads what it writes, also when an output is its input
  std::vector<float> a(count), b(passes > 1 ? count : 0), va(count), vb(passes > 1 ? count : 0), T(count);
  const float *src = value, *vsrc = variance;
  for (int i = 0; i < passes; ++i) {
    float* dst = (i & 1) ? b.data() : a.data();
    float* vdst = (i & 1) ? vb.data() : va.data();
    const float vmax = p->base.value_max_diff * ldexpf(1.0f, -i);     // one product by an exact power of two; +INFINITY stays
    threshold_pass(*p, vsrc, position4, T.data());
    filter_pass(*p, 1 << i, vmax, T.data(), src, vsrc, position4, normal4, dst, vdst);
    src = dst;
    vsrc = vdst;
  }
  memcpy(out_value, src, count * sizeof(float));
  if (out_variance) memcpy(out_variance, vsrc, count * sizeof(float));
  return RT_OK;
}

}  // extern "C"
