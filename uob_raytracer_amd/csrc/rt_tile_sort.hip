// rt_tile_sort.hip — host arithmetic on the scene's triangles: the vertices' box, and the order and per-tile data of the
// mesh kernel's tiled copy (rt_kernel_mesh.hip).  No device code; built with the library's flags: with -ffp-contract=off the
// tile data are the same floats as rt_scene_update.hip's refit computes on the device.
#include <algorithm>
#include <cmath>
#include <utility>

#include "rt_host.h"

namespace uobrt {

void vertex_box(const float* vertices4, int n, float lo[3], float hi[3]) {
  for (int k = 0; k < 3; ++k) { lo[k] = 3.0e38f; hi[k] = -3.0e38f; }
  for (size_t v = 0; v < (size_t)n * 3; ++v)
    for (int k = 0; k < 3; ++k) {
      lo[k] = fminf(lo[k], vertices4[4 * v + k]);
      hi[k] = fmaxf(hi[k], vertices4[4 * v + k]);
    }
}

// 10 bits -> every third bit
static uint32_t spread3(uint32_t v) {
  v &= 1023u;
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// The mesh kernel's copy of the scene (rt_kernel_mesh.hip): the triangle ORDER is a free choice there — shadow tests are
// any-hit, and the closest-hit search resolves equal t by the ORIGINAL index (the reference's loop order, kernels.cl:120)
// — so the triangles are sorted into spatially compact tiles of 64: a task's rays then meet few tiles.  Triangles whose
// extent exceeds a quarter of the scene's (walls) come first, the rest in Morton order of their centroids.
// Three parts, shared by rt_init and rt_update_scene(RT_UPDATE_REORDER): the order (tiled_order), the per-tile data for an
// order (tile_data_host; rt_scene_update.hip's refit computes the same floats on the device) and the upload (rt_scene.hip upload_tiled).
// Returns orig: orig[j] = original index of the triangle at tiled position j.
std::vector<int> tiled_order(const float* v4, int n, bool morton) {
  float lo[3], hi[3];
  vertex_box(v4, n, lo, hi);
  float ext = 0.0f;
  for (int k = 0; k < 3; ++k) ext = fmaxf(ext, hi[k] - lo[k]);
  const float inv = ext > 0.0f ? 1023.0f / ext : 0.0f;
  std::vector<std::pair<uint32_t, int>> key((size_t)n);
  for (int i = 0; i < n; ++i) {
    const float* a = v4 + (size_t)12 * i;
    float tl[3], th[3];
    for (int k = 0; k < 3; ++k) { tl[k] = fminf(fminf(a[k], a[4 + k]), a[8 + k]); th[k] = fmaxf(fmaxf(a[k], a[4 + k]), a[8 + k]); }
    const float te = fmaxf(fmaxf(th[0] - tl[0], th[1] - tl[1]), th[2] - tl[2]);
    uint32_t code = 0u;
    if (!(te > 0.25f * ext)) {
      uint32_t q[3];
      for (int k = 0; k < 3; ++k) {
        const float f = (0.5f * (tl[k] + th[k]) - lo[k]) * inv;
        q[k] = f >= 0.0f ? (f < 1023.0f ? (uint32_t)f : 1023u) : 0u;
      }
      code = 0x40000000u | spread3(q[0]) | (spread3(q[1]) << 1) | (spread3(q[2]) << 2);
    }
    key[(size_t)i] = std::make_pair(code, i);
  }
  std::stable_sort(key.begin(), key.end(), [](const std::pair<uint32_t, int>& x, const std::pair<uint32_t, int>& y) { return x.first < y.first; });
  // UOB_RT_TILE_ORDER=kd (default, Tuning::tile_morton): the small triangles are not left in Morton order (runs of 64 along a space-filling curve
  // jump between octants: a quarter of this round's test mesh's tiles had a normal-cone chord above 0.8) but split top-down at
  // the median of the longest axis of their centroids' box, every cut on a tile boundary, until a range is one tile: compact
  // boxes, compact normal cones.  =morton keeps round 2's order (A/B).  The order is a free choice (see above).
  {
    int nb = 0;
    while (nb < n && key[(size_t)nb].first == 0u) ++nb;                  // the large triangles, in original order
    if (!morton && n - nb > 64) {
      std::vector<float> cen((size_t)n * 3);
      for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) cen[(size_t)3 * i + k] = (v4[(size_t)12 * i + k] + v4[(size_t)12 * i + 4 + k] + v4[(size_t)12 * i + 8 + k]) * (1.0f / 3.0f);
      std::vector<int> idx((size_t)(n - nb));
      for (int j = nb; j < n; ++j) idx[(size_t)(j - nb)] = key[(size_t)j].second;
      // ranges [b, e) of idx; position p of idx is position nb + p of the tiled order: cuts where (nb + p) % 64 == 0
      std::vector<std::pair<int, int>> stack;
      stack.push_back(std::make_pair(0, n - nb));
      while (!stack.empty()) {
        const int b = stack.back().first, e = stack.back().second;
        stack.pop_back();
        if ((nb + b) / 64 == (nb + e - 1) / 64) continue;               // one tile
        float clo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, chi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
        for (int p = b; p < e; ++p)
          for (int k = 0; k < 3; ++k) { clo[k] = fminf(clo[k], cen[(size_t)3 * idx[(size_t)p] + k]); chi[k] = fmaxf(chi[k], cen[(size_t)3 * idx[(size_t)p] + k]); }
        int ax = 0;
        if (chi[1] - clo[1] > chi[ax] - clo[ax]) ax = 1;
        if (chi[2] - clo[2] > chi[ax] - clo[ax]) ax = 2;
        // the tile boundary nearest to the middle of the range
        const int first_cut = ((nb + b) / 64 + 1) * 64 - nb, last_cut = ((nb + e - 1) / 64) * 64 - nb;
        int m = ((nb + (b + e) / 2 + 32) / 64) * 64 - nb;
        m = m < first_cut ? first_cut : (m > last_cut ? last_cut : m);
        std::nth_element(idx.begin() + b, idx.begin() + m, idx.begin() + e,
                         [&](int x, int y) { return cen[(size_t)3 * x + ax] < cen[(size_t)3 * y + ax] || (cen[(size_t)3 * x + ax] == cen[(size_t)3 * y + ax] && x < y); });
        stack.push_back(std::make_pair(b, m));
        stack.push_back(std::make_pair(m, e));
      }
      for (int j = nb; j < n; ++j) key[(size_t)j].second = idx[(size_t)(j - nb)];
    }
  }
  std::vector<int> orig((size_t)n);
  for (int j = 0; j < n; ++j) orig[(size_t)j] = key[(size_t)j].second;
  return orig;
}

// The tiles' data for the order orig, 12 floats per tile (rt_device.h FrameParams::tile_box), from the ORIGINAL-order vertices
std::vector<float> tile_data_host(const float* v4, const int* orig, int n) {
  const int ntiles = mesh_tiles(n);
  std::vector<float> box((size_t)ntiles * 12);
  for (int t = 0; t < ntiles; ++t) { for (int k = 0; k < 3; ++k) { box[(size_t)12 * t + k] = 3.0e38f; box[(size_t)12 * t + 4 + k] = -3.0e38f; } box[(size_t)12 * t + 3] = box[(size_t)12 * t + 7] = 0.0f; }
  for (int j = 0; j < n; ++j) {
    const int i = orig[j];
    float* b = &box[(size_t)12 * (j / 64)];
    for (int v = 0; v < 3; ++v)
      for (int k = 0; k < 3; ++k) { b[k] = fminf(b[k], v4[(size_t)12 * i + 4 * v + k]); b[4 + k] = fmaxf(b[4 + k], v4[(size_t)12 * i + 4 * v + k]); }
  }
  // Per tile, for the bounce rays' tile pre-test (rt_kernel_mesh.hip tile_clear_for_bundle), in double from the float vertices:
  //   lo.w  eta   = max over the tile's triangles of max(|e1|, |e2|, |e2 - e1|) / |e1 x e2|   (inverse altitudes)
  //   hi.w  emax  = max edge length
  //   third float4: unit axis of the triangles' normals (signs aligned) | chi = max |n_T - axis|_2 (chord of the normal cone)
  // A tile with a degenerate triangle gets chi = 4: never certified clear, always visited.  (rt_scene_update.hip
  // rt_scene_refit is the same arithmetic, one lane per triangle: change both together.)
  for (int t = 0; t < ntiles; ++t) {
    const int j0 = t * 64, j1 = (j0 + 64 < n) ? j0 + 64 : n;
    double ax[3] = {0, 0, 0}, eta = 0.0, emax = 0.0;
    bool degenerate = false;
    std::vector<double> nn((size_t)(j1 - j0) * 3);
    for (int j = j0; j < j1; ++j) {
      const float* a = v4 + (size_t)12 * orig[j];
      const double e1[3] = {(double)a[4] - a[0], (double)a[5] - a[1], (double)a[6] - a[2]};
      const double e2[3] = {(double)a[8] - a[0], (double)a[9] - a[1], (double)a[10] - a[2]};
      double cr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
      const double l1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]), l2 = sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
      const double lc = sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
      if (!(lc > 1e-30) || !(l1 > 0) || !(l2 > 0) || !(lc >= 1e-9 * l1 * l2)) { degenerate = true; break; }
      const double l3 = sqrt((e2[0] - e1[0]) * (e2[0] - e1[0]) + (e2[1] - e1[1]) * (e2[1] - e1[1]) + (e2[2] - e1[2]) * (e2[2] - e1[2]));
      const double le = fmax(fmax(l1, l2), l3);
      eta = fmax(eta, le / lc);
      emax = fmax(emax, le);
      double* q = &nn[(size_t)(j - j0) * 3];
      for (int k = 0; k < 3; ++k) q[k] = cr[k] / lc;
      if (j > j0 && q[0] * nn[0] + q[1] * nn[1] + q[2] * nn[2] < 0) for (int k = 0; k < 3; ++k) q[k] = -q[k];   // align with the first
      for (int k = 0; k < 3; ++k) ax[k] += q[k];
    }
    float* b = &box[(size_t)12 * t];
    const double la = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    double chi = 4.0;
    if (!degenerate && la > 1e-12) {
      for (int k = 0; k < 3; ++k) ax[k] /= la;
      chi = 0.0;
      for (int j = j0; j < j1; ++j) {
        const double* q = &nn[(size_t)(j - j0) * 3];
        const double dx = q[0] - ax[0], dy = q[1] - ax[1], dz = q[2] - ax[2];
        chi = fmax(chi, sqrt(dx * dx + dy * dy + dz * dz));
      }
    } else {
      ax[0] = 1.0; ax[1] = ax[2] = 0.0; eta = 1e30; emax = 1e30;
    }
    b[3] = (float)(eta * 1.0001); b[7] = (float)(emax * 1.0001);
    b[8] = (float)ax[0]; b[9] = (float)ax[1]; b[10] = (float)ax[2]; b[11] = (float)(chi * 1.0001 + 1e-6);
  }
  return box;
}

}  // namespace uobrt
