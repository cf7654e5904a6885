// screen.cpp — headless implementation of the reference's SDLauxiliary.h surface (see screen.h).
#include "screen.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <iostream>
#include <string>

screen* InitializeSDL(int width, int height, bool /*fullscreen*/) {
  screen* s = new screen;
  memset(s, 0, sizeof *s);
  s->width = width;
  s->height = height;
  s->buffer = new uint32_t[(size_t)width * height];           // SDLauxiliary.h:105-106
  memset(s->buffer, 0, (size_t)width * height * sizeof(uint32_t));
  return s;
}

// SDLauxiliary.h:150-162: clamp(255*c, 0, 255) truncated, alpha 128
void PutPixelSDL(screen* s, int x, int y, float r, float g, float b) {
  if (x < 0 || x >= s->width || y < 0 || y >= s->height) {
    std::cout << "apa" << std::endl;
    return;
  }
  auto q = [](float c) { float v = 255 * c; v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v); return (uint32_t)v; };
  s->buffer[y * s->width + x] = (128u << 24) + (q(r) << 16) + (q(g) << 8) + q(b);
}

void SDL_Renderframe(screen* s) { s->frames_presented++; }    // SDLauxiliary.h:65-71 blits; headless: count

void KillSDL(screen* s) {                                     // SDLauxiliary.h:56-63
  delete[] s->buffer;
  delete s;
}

// SDLauxiliary.h:24-54: SDL_CreateRGBSurfaceFrom(buffer, ARGB masks) + SDL_SaveBMP
void SDL_SaveImage(screen* s, const char* filename) {
  FILE* f = fopen(filename, "wb");
  if (!f) {
    std::cout << "Failed to save image: cannot open " << filename << std::endl;
    exit(1);
  }
  const uint32_t w = (uint32_t)s->width, h = (uint32_t)s->height, image = w * h * 4, off = 14 + 108;
  uint8_t hdr[14 + 108];
  memset(hdr, 0, sizeof hdr);
  auto put32 = [&](int at, uint32_t v) { memcpy(hdr + at, &v, 4); };
  auto put16 = [&](int at, uint16_t v) { memcpy(hdr + at, &v, 2); };
  hdr[0] = 'B'; hdr[1] = 'M';
  put32(2, off + image); put32(10, off);
  put32(14, 108);                       // BITMAPV4HEADER
  put32(18, w); put32(22, h);           // positive height: bottom-up
  put16(26, 1); put16(28, 32);
  put32(30, 3);                         // BI_BITFIELDS
  put32(34, image);
  put32(54, 0x00FF0000u); put32(58, 0x0000FF00u); put32(62, 0x000000FFu); put32(66, 0xFF000000u);   // R G B A masks
  put32(70, 0x57696E20u);               // LCS_WINDOWS_COLOR_SPACE, as SDL writes
  fwrite(hdr, 1, sizeof hdr, f);
  for (uint32_t y = 0; y < h; ++y) fwrite(s->buffer + (size_t)(h - 1 - y) * w, 4, w, f);
  fclose(f);
}

// A fixed hash of the primitive id (-2 sphere, -1 miss, >= 0 triangle) to an opaque colour: Knuth's multiplicative hash,
// its top 24 bits.  (A bijection on 32 bits; two ids share a colour only if their difference times the constant falls
// within 256 of a multiple of 2^32 — no two ids below 3 000 apart do.)
uint32_t aov_id_colour(int32_t id) { return 0xFF000000u | (((uint32_t)(id + 2) * 2654435761u) >> 8); }

void SaveAovImages(const char* prefix, int width, int height, const int32_t* prim, const float* depth, const float* normal4) {
  screen* s = InitializeSDL(width, height, false);
  const size_t count = (size_t)width * height;
  auto q = [](float c) { float v = 255 * c; v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v); return (uint32_t)v; };
  auto grey = [&](float r, float g, float b) { return (255u << 24) + (q(r) << 16) + (q(g) << 8) + q(b); };
  float lo = INFINITY, hi = -INFINITY;
  for (size_t i = 0; i < count; ++i)
    if (std::isfinite(depth[i])) { lo = depth[i] < lo ? depth[i] : lo; hi = depth[i] > hi ? depth[i] : hi; }
  for (size_t i = 0; i < count; ++i) {
    const float g = !std::isfinite(depth[i]) ? 0.0f : (hi > lo ? (hi - depth[i]) / (hi - lo) : 1.0f);
    s->buffer[i] = grey(g, g, g);
  }
  SDL_SaveImage(s, (std::string(prefix) + "_depth.bmp").c_str());
  for (size_t i = 0; i < count; ++i)
    s->buffer[i] = grey(0.5f * normal4[4 * i] + 0.5f, 0.5f * normal4[4 * i + 1] + 0.5f, 0.5f * normal4[4 * i + 2] + 0.5f);
  SDL_SaveImage(s, (std::string(prefix) + "_normal.bmp").c_str());
  for (size_t i = 0; i < count; ++i) s->buffer[i] = aov_id_colour(prim[i]);
  SDL_SaveImage(s, (std::string(prefix) + "_id.bmp").c_str());
  KillSDL(s);
}
