// temporal_host_sanitize.cpp — rtw_temporal's and rtw_denoise_counts' host loops under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a program of its own: no GPU, no Python, no librtw_amd.so.  It compiles the two host
// sources themselves and supplies the few functions they take from the rest of the library (the error message, the
// image checks, the two enqueue calls, which it never reaches).  From the repository's root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Wno-unused-result
//     -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ scripts/temporal_host_sanitize.cpp
//     raytracer-weekend_amd/csrc/rtw_temporal.cpp raytracer-weekend_amd/csrc/rtw_denoise.cpp
//     -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -o temporal_host_sanitize && ./temporal_host_sanitize
// It runs the 37x21 and 2x2 cases: a camera pair a pixel of parallax apart over a floor and a wall, with and without
// history, every optional triple NULL, a tile table with an empty tile, in place and out of place, planted NaN,
// infinite and zero history pixels, a history camera facing away; every buffer is a heap block of exactly the stated
// size, so a read or write one float beyond it is reported.  Exit status 0 and "ok" mean the sanitizers saw nothing.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/rtw.h"
#include "../raytracer-weekend_amd/csrc/rtw_scene.hpp"

namespace rtw {
static char g_err[512];
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
int check_image_min(uint32_t w, uint32_t h) { return w < 2 || h < 2 ? fail(RTW_EINVAL, "image under 2x2") : RTW_OK; }
int check_image_max(uint32_t w, uint32_t h) {
  return w > 65536u || h > 65536u ? fail(RTW_EINVAL, "image over 65536 a side") : RTW_OK;
}
int enqueue_denoise(const float*, const float*, const float*, const float*, const float*, const float*, uint32_t,
                    uint32_t, uint32_t, const uint32_t*, uint32_t, float, float, float, float*, void*, hipStream_t) {
  return fail(RTW_ENODEV, "no device in this program");
}
int enqueue_temporal(const TemporalArgs&, hipStream_t) { return fail(RTW_ENODEV, "no device in this program"); }
}  // namespace rtw

namespace {

// a pinhole camera at `from` looking down -z: vfov 50 degrees, focus distance 1
rtw_camera camera(float x, float y, float z, float aspect, bool away) {
  rtw_camera c;
  memset(&c, 0, sizeof c);
  const float hh = 2.0f * tanf(25.0f * 3.14159265f / 180.0f), ww = hh * aspect, s = away ? -1.0f : 1.0f;
  c.origin[0] = x, c.origin[1] = y, c.origin[2] = z;
  c.w[2] = s, c.u[0] = s, c.v[1] = 1.0f;
  c.horizontal[0] = s * ww, c.vertical[1] = hh;
  for (int k = 0; k < 3; ++k)
    c.lower_left_corner[k] = c.origin[k] - 0.5f * c.horizontal[k] - 0.5f * c.vertical[k] - c.w[k];
  c.time1 = 1.0f;
  return c;
}

struct Frame {
  std::vector<float> sum, sq, albedo, normal, depth, count;
};

// n samples through every pixel centre of a floor (y = 0) and a wall (z = -6, up to y = 2.6); above the wall nothing
Frame frame(const rtw_camera& c, uint32_t w, uint32_t h, float n) {
  const size_t px = (size_t)w * h;
  Frame f;
  f.sum.resize(px * 3), f.sq.resize(px * 3), f.albedo.resize(px * 3), f.normal.resize(px * 3), f.depth.resize(px * 2);
  f.count.assign(px, n);
  uint32_t rng = 12345u;
  for (uint32_t row = 0; row < h; ++row)
    for (uint32_t i = 0; i < w; ++i) {
      const size_t p = (size_t)row * w + i;
      const float s = ((float)i + 0.5f) / (float)(w - 1), v = ((float)(h - 1 - row) + 0.5f) / (float)(h - 1);
      float d[3];
      for (int k = 0; k < 3; ++k)
        d[k] = c.lower_left_corner[k] + s * c.horizontal[k] + v * c.vertical[k] - c.origin[k];
      float t = -1.0f, nrm[3] = {0, 0, 0};
      const float tf = -c.origin[1] / d[1], tw = (-6.0f - c.origin[2]) / d[2];
      if (tf > 0 && c.origin[2] + tf * d[2] > -6.0f) t = tf, nrm[1] = 1.0f;
      else if (tw > 0 && c.origin[1] + tw * d[1] > 0 && c.origin[1] + tw * d[1] < 2.6f) t = tw, nrm[2] = 1.0f;
      for (int k = 0; k < 3; ++k) {
        rng = rng * 1664525u + 1013904223u;
        const float x = 0.2f + (float)(rng >> 8) / 16777216.0f;
        f.sum[p * 3 + k] = n * x, f.sq[p * 3 + k] = n * x * x, f.albedo[p * 3 + k] = n * 0.5f;
        f.normal[p * 3 + k] = t > 0 ? n * nrm[k] : 0.0f;
      }
      f.depth[p * 2] = t > 0 ? n * t : 0.0f, f.depth[p * 2 + 1] = t > 0 ? n : 0.0f;
    }
  return f;
}

int failures = 0;
void expect(int rc, const char* what) {
  if (rc != RTW_OK) {
    printf("%s: %d %s\n", what, rc, rtw::g_err);
    ++failures;
  }
}

void run(uint32_t w, uint32_t h) {
  const float aspect = (float)w / (float)h;
  const size_t px = (size_t)w * h;
  const rtw_camera cam = camera(0.0f, 1.6f, 2.0f, aspect, false), moved = camera(0.25f, 1.6f, 2.0f, aspect, false),
                   back = camera(0.25f, 1.6f, 2.0f, aspect, true);
  Frame hist = frame(moved, w, h, 6.5f);
  const float nan = nanf(""), inf = INFINITY;
  hist.sum[0] = nan, hist.sum[3 * (px - 1)] = inf, hist.count[px / 2] = 0.0f, hist.count[px / 3] = nan;
  hist.depth[2 * (px / 4) + 1] = 0.0f, hist.depth[2 * (px / 5)] = nan;
  std::vector<uint32_t> tiles((size_t)((w + 7) / 8) * ((h + 7) / 8), 2u);
  tiles[tiles.size() / 2] = 0u;
  double sum = 0.0;
  for (int variant = 0; variant < 6; ++variant) {
    const bool with_hist = variant != 1, bare = variant == 2, table = variant == 3, in_place = variant == 4;
    const rtw_camera& hc = variant == 5 ? back : moved;
    Frame cur = frame(cam, w, h, 2.0f), out;
    out.sum.resize(px * 3), out.sq.resize(px * 3), out.albedo.resize(px * 3), out.normal.resize(px * 3);
    out.depth.resize(px * 2), out.count.resize(px);
    Frame& o = in_place ? cur : out;
    expect(rtw_temporal(cur.sum.data(), bare ? nullptr : cur.sq.data(), bare ? nullptr : cur.albedo.data(),
                        bare ? nullptr : cur.normal.data(), cur.depth.data(), w, h, table ? 0u : 2u,
                        table ? tiles.data() : nullptr, &cam, hist.sum.data(), hist.sq.data(), hist.albedo.data(),
                        hist.normal.data(), hist.depth.data(), with_hist ? hist.count.data() : nullptr, &hc, 8.0f, 0.05f,
                        0.9f, o.sum.data(), bare ? nullptr : o.sq.data(), bare ? nullptr : o.albedo.data(),
                        bare ? nullptr : o.normal.data(), o.depth.data(), out.count.data()),
           "rtw_temporal");
    std::vector<float> mean(px * 3);
    for (uint32_t it : {0u, 3u, 6u}) {
      expect(rtw_denoise_counts(o.sum.data(), bare ? nullptr : o.sq.data(), bare ? nullptr : o.albedo.data(),
                                bare ? nullptr : o.normal.data(), o.depth.data(), out.count.data(), w, h, it, 4.0f, 0.5f,
                                0.1f, mean.data()),
             "rtw_denoise_counts");
      for (float m : mean)
        if (m == m && m < 1e30f) sum += m;
    }
  }
  printf("%ux%u: checksum %.6f\n", w, h, sum);
}

}  // namespace

int main() {
  run(37, 21);
  run(2, 2);
  // and one failing check each, so that the shared check functions run too
  float x[12] = {0};
  if (rtw_temporal(nullptr, nullptr, nullptr, nullptr, x, 2, 2, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                   nullptr, nullptr, nullptr, 1.0f, 0.05f, 0.9f, x, nullptr, nullptr, nullptr, x, x) != RTW_EINVAL)
    ++failures;
  if (rtw_denoise_counts(x, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 2, 1, 4.0f, 0.5f, 0.1f, x) != RTW_EINVAL)
    ++failures;
  printf(failures ? "FAILED: %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
