// rtw_console.cpp — the build's console_app (console_app/src/main.rs:15-96) on the GPU core.
//
//   rtw_console <scene> [-w|--width 400] [-a|--aspect-ratio 1.7777778] [-s|--samples-per-pixel 100]
//               [--seed 0] [--models models] [--out render] [--progressive STEP] [--adaptive THRESHOLD [--min-spp 16]]
//               [--features] [--denoise [ITERATIONS]] [--temporal] [--ao RADIUS [--ao-rays K]]
// Same Opts and defaults (main.rs:15-26), height = round(width / aspect) (:33), camera
// aspect = width / height as f32 (:38-41), tonemap (:68-90), PNG to render/image_0000.png (:92-94).
// --progressive (no counterpart in console_app) renders each frame through rtw_render_progressive: the PNG is rewritten
// after every step, and its last version is the one-shot frame's file byte for byte.
// --adaptive renders each frame through rtw_render_adaptive with -s as the most samples a tile gets, and writes the PNG
// through rtw_tonemap_tiles: every 8x8 tile is the one-shot frame's at the sample count it stopped at.
// --features writes, beside each frame's PNG, the denoiser's guides from rtw_render_features at the frame's spp:
// albedo_NNNN.png (rtw_tonemap of the albedo sums) and normal_NNNN.png (the summed normal's direction, 0.5 + 0.5 n).
// --denoise writes, beside each frame's PNG, image_NNNN_denoised.png: the frame through rtw_denoise (the edge-avoiding
// a-trous filter of include/rtw.h on the host arrays the render calls return, rtw.hpp's default sigmas) and rtw_tonemap.
// --temporal renders frame k with seed + k and writes, beside each frame's PNG, image_NNNN_temporal.png: the frame
// accumulated onto the reprojected frames before it (rtw_temporal, rtw.hpp's defaults), denoised (rtw_denoise_counts,
// the default sigmas and --denoise's ITERATIONS) and tonemapped, all on host arrays.
// --ao writes, beside each frame's PNG, ao_NNNN.png: the ambient occlusion of the frame's spp camera rays per pixel
// (rtw_render_ao, K rays per hit up to RADIUS, `inf` for sky visibility) as the grey open / cast, white where nothing was
// hit, through rtw_tonemap with spp = 1.
#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "rtw.hpp"

static void put32(std::vector<uint8_t>& v, uint32_t x) {
  for (int s = 24; s >= 0; s -= 8) v.push_back((uint8_t)(x >> s));
}
static void chunk(FILE* f, const char* type, const std::vector<uint8_t>& data) {
  std::vector<uint8_t> buf;
  put32(buf, (uint32_t)data.size());
  buf.insert(buf.end(), type, type + 4);
  buf.insert(buf.end(), data.begin(), data.end());
  uint32_t crc = (uint32_t)crc32(0, buf.data() + 4, (uInt)(buf.size() - 4));
  put32(buf, crc);
  fwrite(buf.data(), 1, buf.size(), f);
}
static bool write_png(const char* path, const uint8_t* rgb, uint32_t w, uint32_t h) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
  fwrite(sig, 1, 8, f);
  std::vector<uint8_t> ihdr;
  put32(ihdr, w);
  put32(ihdr, h);
  ihdr.insert(ihdr.end(), {8, 2, 0, 0, 0});
  chunk(f, "IHDR", ihdr);
  std::vector<uint8_t> raw;
  raw.reserve((size_t)h * (w * 3 + 1));
  for (uint32_t y = 0; y < h; ++y) {
    raw.push_back(0);
    raw.insert(raw.end(), rgb + (size_t)y * w * 3, rgb + (size_t)(y + 1) * w * 3);
  }
  uLongf n = compressBound((uLong)raw.size());
  std::vector<uint8_t> z(n);
  compress2(z.data(), &n, raw.data(), (uLong)raw.size(), 6);
  z.resize(n);
  chunk(f, "IDAT", z);
  chunk(f, "IEND", {});
  return fclose(f) == 0;
}

// The frame's mean relative standard error from the two sums, n samples in (--help states the definition)
static double mean_rel_stderr(const float* sum, const float* sq, size_t n_pixels, uint32_t n) {
  static const double wgt[3] = {0.2126, 0.7152, 0.0722};
  double tot = 0.0;
  size_t lit = 0;
  for (size_t p = 0; p < n_pixels; ++p) {
    double mean = 0.0, se = 0.0;
    for (int c = 0; c < 3; ++c) {
      const double m = (double)sum[p * 3 + c] / n;
      const double v = fmax(0.0, (double)sq[p * 3 + c] / n - m * m) * n / (n - 1.0);
      mean += wgt[c] * m;
      se += wgt[c] * sqrt(v / n);
    }
    if (mean != 0.0 && mean == mean && se == se) {
      tot += se / fabs(mean);
      ++lit;
    }
  }
  return lit ? tot / (double)lit : 0.0;
}

// --features' normal image: per channel u8(255.999 * clamp(0.5 + 0.5 * N_c / |N|, 0, 0.999)) of the pixel's summed
// normal N; a zero N gives 0.5
static void normal_rgb8(const float* n, size_t n_pixels, uint8_t* rgb) {
  for (size_t p = 0; p < n_pixels; ++p) {
    const float x = n[p * 3], y = n[p * 3 + 1], z = n[p * 3 + 2];
    const float len = sqrtf(x * x + y * y + z * z);
    for (int c = 0; c < 3; ++c) {
      float v = len > 0.0f ? 0.5f + 0.5f * (n[p * 3 + c] / len) : 0.5f;
      v = v < 0.0f ? 0.0f : (v > 0.999f ? 0.999f : v);
      rgb[p * 3 + c] = v == v ? (uint8_t)(255.999f * v) : (uint8_t)0;
    }
  }
}

int main(int argc, char** argv) {
  std::string scene, models = "models", out_dir = "render";
  uint32_t width = 400, spp = 100, step = 0, min_spp = 16, ao_rays = 1;
  bool progressive = false, adaptive = false, features = false, denoise = false, temporal = false, ao = false;
  float ao_radius = 0.0f;
  uint32_t denoise_iterations = rtw::DENOISE_ITERATIONS;
  float threshold = 0.0f;
  double aspect = 1.7777778;
  uint64_t seed = 0;
  for (int k = 1; k < argc; ++k) {
    std::string a = argv[k];
    auto next = [&](const char* what) -> const char* {
      if (k + 1 >= argc) { fprintf(stderr, "missing value for %s\n", what); exit(2); }
      return argv[++k];
    };
    if (a == "-w" || a == "--width") width = (uint32_t)atoi(next("--width"));
    else if (a == "-a" || a == "--aspect-ratio") aspect = atof(next("--aspect-ratio"));
    else if (a == "-s" || a == "--samples-per-pixel") spp = (uint32_t)atoi(next("--samples-per-pixel"));
    else if (a == "--seed") seed = strtoull(next("--seed"), nullptr, 0);
    else if (a == "--models") models = next("--models");
    else if (a == "--out") out_dir = next("--out");
    else if (a == "--progressive") { progressive = true; step = (uint32_t)atoi(next("--progressive")); }
    else if (a == "--adaptive") { adaptive = true; threshold = (float)atof(next("--adaptive")); }
    else if (a == "--features") features = true;
    else if (a == "--denoise") {
      denoise = true;
      if (k + 1 < argc && isdigit((unsigned char)argv[k + 1][0])) denoise_iterations = (uint32_t)atoi(argv[++k]);
    }
    else if (a == "--temporal") temporal = true;
    else if (a == "--ao") { ao = true; ao_radius = (float)atof(next("--ao")); }
    else if (a == "--ao-rays") ao_rays = (uint32_t)atoi(next("--ao-rays"));
    else if (a == "--min-spp") min_spp = (uint32_t)atoi(next("--min-spp"));
    else if (a == "-h" || a == "--help") {
      printf("usage: rtw_console <jumpy-balls|two-spheres|two-perlin-spheres|earth|simple-light|cornell-box|"
             "smokey-cornell-box|book2-final-scene|animated-book2-final-scene|simple-triangle|wavefront-cow-obj|"
             "wavefront-suspension-obj|textured-monument> [-w W] [-a ASPECT] [-s SPP] [--seed N] [--models DIR] "
             "[--out DIR] [--progressive STEP] [--adaptive THRESHOLD [--min-spp N]] [--features] "
             "[--denoise [ITERATIONS]] [--temporal] [--ao RADIUS [--ao-rays K]]\n"
             "  --progressive STEP  render each frame in growing steps (1, 2, 4, ... samples while the doubled count is\n"
             "      within STEP, then STEP at a time; 0 = doubling to the end); after every step the frame's PNG is\n"
             "      rewritten and the samples done and the mean relative standard error are printed.  That error, from\n"
             "      the per-pixel sums S and sums of squares Q over n samples: per channel the mean m = S / n and the\n"
             "      variance v = max(0, Q / n - m^2) n / (n - 1); the luminance Y = 0.2126 R + 0.7152 G + 0.0722 B has\n"
             "      mean sum_c w_c m_c and standard error sum_c w_c sqrt(v_c / n) (the channels taken as fully\n"
             "      correlated: an upper bound); a pixel's relative error is the second over the first, and the frame's\n"
             "      is its average over the pixels whose mean luminance is not zero (n/a at n = 1).\n"
             "  --adaptive THRESHOLD [--min-spp N]  a sample count per 8x8 tile: every tile gets N (default 16) samples,\n"
             "      then 2 N, 4 N, ... up to SPP, and stops at the first count at which its noise estimate (rtw.h: the\n"
             "      tile's root mean variance of the mean over its mean brightness + 0.03) is <= THRESHOLD.  Prints the\n"
             "      number of tiles per sample count.\n"
             "  --features  also write the denoiser's guides of each frame, first-hit features summed over the pixel's\n"
             "      SPP camera rays: albedo_NNNN.png (the albedo sums through the image's tonemap) and normal_NNNN.png\n"
             "      (per channel 255.999 clamp(0.5 + 0.5 N_c / |N|, 0, 0.999) of the summed normal N; 0.5 where N = 0).\n"
             "  --denoise [ITERATIONS]  also write image_NNNN_denoised.png: the frame's sums, sums of squares and guides\n"
             "      through the edge-avoiding a-trous filter (rtw.h; ITERATIONS passes, default 5, at most 10; sigma_l 4,\n"
             "      sigma_n 0.5, sigma_z 0.1), on the host arrays the render calls return.  Meant for few samples (-s 4).\n"
             "      Not with --adaptive.\n"
             "  --temporal  render frame k with seed N + k (one seed for every frame would repeat each pixel's noise) and\n"
             "      also write image_NNNN_temporal.png: the frame accumulated onto the frames before it, reprojected\n"
             "      through each pixel's mean first-hit depth onto the frame's camera (rtw.h; at most 32 SPP effective\n"
             "      samples of history, depth within 5%%, normals within cos 0.9), then through the filter of --denoise\n"
             "      with the accumulated sample count of each pixel.  Meant for few samples (-s 2) and a scene with\n"
             "      several cameras (animated-book2-final-scene).  Not with --adaptive.\n"
             "  --ao RADIUS [--ao-rays K]  also write ao_NNNN.png, the frame's ambient occlusion: from the first hit of\n"
             "      each of the pixel's SPP camera rays, K (default 1, at most 256) cosine-distributed rays; the grey value\n"
             "      is the share of them that meet nothing within RADIUS (inf: that see the sky), white where the pixel hit\n"
             "      nothing, through the image's tonemap.  Meant for few samples (-s 4).  Not with --adaptive.\n");
      return 0;
    } else if (scene.empty()) scene = a;
    else { fprintf(stderr, "unexpected argument '%s'\n", a.c_str()); return 2; }
  }
  if (scene.empty()) { fprintf(stderr, "missing scene subcommand (try --help)\n"); return 2; }
  if (denoise && adaptive) { fprintf(stderr, "--denoise is not combined with --adaptive\n"); return 2; }
  if (temporal && adaptive) { fprintf(stderr, "--temporal is not combined with --adaptive\n"); return 2; }
  if (ao && adaptive) { fprintf(stderr, "--ao is not combined with --adaptive\n"); return 2; }
  const uint32_t height = (uint32_t)llround((double)width / aspect);  // main.rs:33 (f64 round)
  try {
    rtw::World world;
    rtw::Camera cam;
    rtw::Color bg;
    const float cam_aspect = (float)width / (float)height;  // main.rs:38-41
    world.preset(scene, cam_aspect, seed, models, cam, bg);
    world.commit();  // flattened and uploaded once, reused by every camera (main.rs:47-56)
    const std::vector<rtw::Camera> cams = rtw::World::preset_cameras(scene, cam_aspect, models);
    mkdir(out_dir.c_str(), 0755);
    rtw::AccumulatedFrame history;  // --temporal: the accumulated frame before this one (empty: none yet)
    const bool want_sq = denoise || temporal;
    for (size_t frame = 0; frame < cams.size(); ++frame) {
      rtw::Raytracer rt(world, cams[frame], bg, width, height, spp, temporal ? seed + frame : seed);
      rtw_stats st;
      char name[32];
      snprintf(name, sizeof name, "/image_%04zu.png", frame);  // main.rs:92-94
      std::string path = out_dir + name;
      std::vector<uint8_t> img((size_t)width * height * 3);
      std::vector<float> dn_sum, dn_sq;  // --denoise, --temporal: the finished frame's sums and sums of squares
      if (progressive || want_sq) {  // (without --progressive: that call for its squares; only the last step is written)
        const size_t n3 = (size_t)width * height * 3;
        const int rc = rt.render_progressive([&](const float* sum, const float* sq, uint32_t done) {
          if (want_sq && done == spp) {
            dn_sum.assign(sum, sum + n3);
            dn_sq.assign(sq, sq + n3);
          }
          if (!progressive && done != spp) return 0;
          if (rtw_tonemap(sum, width * height, done, img.data()) != RTW_OK) return 1;  // (nothing throws through C)
          if (!write_png(path.c_str(), img.data(), width, height)) return 1;
          if (!progressive) return 0;
          if (done > 1) printf("  %u spp: mean relative standard error %.4f\n", done,
                               mean_rel_stderr(sum, sq, (size_t)width * height, done));
          else printf("  %u spp: mean relative standard error n/a\n", done);
          fflush(stdout);
          return 0;
        }, progressive ? step : 0, &st);
        if (rc) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
      } else if (adaptive) {
        const rtw::AdaptiveFrame fr = rt.render_adaptive(threshold, std::min(min_spp, spp), &st);
        rtw::check(rtw_tonemap_tiles(fr.sums.data(), width, height, fr.tile_samples.data(), img.data()));
        if (!write_png(path.c_str(), img.data(), width, height)) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
        std::map<uint32_t, size_t> hist;
        for (uint32_t n : fr.tile_samples) ++hist[n];
        for (const auto& kv : hist) printf("  %u spp: %zu tiles\n", kv.first, kv.second);
      } else {
        std::vector<float> sums = rt.render_sums(&st);
        rtw::check(rtw_tonemap(sums.data(), width * height, spp, img.data()));
        if (!write_png(path.c_str(), img.data(), width, height)) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
      }
      rtw::FeatureFrame ff;
      if (features || want_sq) ff = rt.render_features();
      if (denoise) {
        const std::vector<float> mean = rtw::denoise(dn_sum.data(), dn_sq.data(), ff.albedo.data(), ff.normal.data(),
                                                     ff.depth.data(), width, height, spp, nullptr, denoise_iterations);
        snprintf(name, sizeof name, "/image_%04zu_denoised.png", frame);
        const std::string dpath = out_dir + name;
        rtw::check(rtw_tonemap(mean.data(), width * height, 1, img.data()));
        if (!write_png(dpath.c_str(), img.data(), width, height)) { fprintf(stderr, "cannot write %s\n", dpath.c_str()); return 1; }
      }
      if (temporal) {
        const rtw::FrameView cur{dn_sum.data(), dn_sq.data(), ff.albedo.data(), ff.normal.data(), ff.depth.data(), nullptr};
        const rtw::FrameView hist = history.view();
        rtw::AccumulatedFrame acc = rtw::temporal(cur, width, height, spp, cams[frame], frame ? &hist : nullptr,
                                                  frame ? &cams[frame - 1] : nullptr,
                                                  (float)(rtw::TEMPORAL_MAX_HISTORY_FRAMES * spp));
        const std::vector<float> mean = rtw::denoise_counts(acc.view(), width, height, denoise_iterations);
        snprintf(name, sizeof name, "/image_%04zu_temporal.png", frame);
        const std::string tpath = out_dir + name;
        rtw::check(rtw_tonemap(mean.data(), width * height, 1, img.data()));
        if (!write_png(tpath.c_str(), img.data(), width, height)) { fprintf(stderr, "cannot write %s\n", tpath.c_str()); return 1; }
        history = std::move(acc);
      }
      if (features) {
        snprintf(name, sizeof name, "/albedo_%04zu.png", frame);
        const std::string apath = out_dir + name;
        rtw::check(rtw_tonemap(ff.albedo.data(), width * height, spp, img.data()));
        if (!write_png(apath.c_str(), img.data(), width, height)) { fprintf(stderr, "cannot write %s\n", apath.c_str()); return 1; }
        snprintf(name, sizeof name, "/normal_%04zu.png", frame);
        const std::string npath = out_dir + name;
        normal_rgb8(ff.normal.data(), (size_t)width * height, img.data());
        if (!write_png(npath.c_str(), img.data(), width, height)) { fprintf(stderr, "cannot write %s\n", npath.c_str()); return 1; }
      }
      if (ao) {
        const std::vector<float> sums = rt.render_ao(ao_rays, ao_radius);
        std::vector<float> grey((size_t)width * height * 3);
        for (size_t p = 0; p < (size_t)width * height; ++p) {
          const float open = sums[p * 2], cast = sums[p * 2 + 1];
          grey[p * 3] = grey[p * 3 + 1] = grey[p * 3 + 2] = cast > 0.0f ? open / cast : 1.0f;
        }
        snprintf(name, sizeof name, "/ao_%04zu.png", frame);
        const std::string opath = out_dir + name;
        rtw::check(rtw_tonemap(grey.data(), width * height, 1, img.data()));
        if (!write_png(opath.c_str(), img.data(), width, height)) { fprintf(stderr, "cannot write %s\n", opath.c_str()); return 1; }
      }
      printf("%s %ux%u %u spp: %.1f ms kernel, %llu rays, %.1f Mrays/s -> %s\n", scene.c_str(), width, height, spp,
             st.kernel_ms, (unsigned long long)st.rays, st.rays / (st.kernel_ms * 1e3), path.c_str());
    }
  } catch (const rtw::Error& e) {
    fprintf(stderr, "error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
