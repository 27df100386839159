// rtw_denoise.cpp — the denoiser's C-ABI calls (include/rtw.h): rtw_denoise_scratch_bytes, rtw_denoise_device (checks,
// then rtw_kernel.hip's enqueue_denoise) and rtw_denoise, the same arithmetic as plain loops over host arrays: what
// rtw_tonemap is beside rtw_tonemap_device; and rtw_denoise_counts_device / rtw_denoise_counts, the same two with a
// sample count per pixel (an accumulated frame, rtw_temporal*'s output) in place of `samples` and the tile table.  The filter is defined in the header operation by operation; this file and
// rtw_denoise_kernel.hpp restate it independently and agree bit for bit (-ffp-contract=off, IEEE division and sqrt;
// tests/test_denoise_abi.py holds this one to a numpy restatement, tests/test_gpu_denoise.py the kernels to both).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <utility>
#include <vector>

#include "../../include/rtw.h"
#include "rtw_scene.hpp"

using namespace rtw;

namespace {

struct Rec {
  float x[3], var;
};
struct Guide {
  float g[3], z;
};

inline float max0(float v) { return v > 0.0f ? v : 0.0f; }  // a NaN gives 0
inline float lum(const Rec& r) { return (0.2126f * r.x[0] + 0.7152f * r.x[1]) + 0.0722f * r.x[2]; }

// the checks both calls share, in the header's order (`scratch`: the device call's third buffer)
int check_denoise(const void* sum, const void* out, bool scratch, uint32_t w, uint32_t h, uint32_t samples,
                  const uint32_t* tile_samples, uint32_t iterations, float sigma_l, float sigma_n, float sigma_z) {
  if (!sum || !out || !scratch) return fail(RTW_EINVAL, "NULL buffer");
  if (int e = check_image_min(w, h)) return e;
  if (int e = check_image_max(w, h)) return e;
  if (samples == 0 && !tile_samples) return fail(RTW_EINVAL, "samples must be > 0 without a tile table");
  if (iterations > 10) return fail(RTW_EINVAL, "iterations %u: at most 10", iterations);
  const float sig[3] = {sigma_l, sigma_n, sigma_z};
  const char* names[3] = {"sigma_l", "sigma_n", "sigma_z"};
  for (int k = 0; k < 3; ++k)
    if (!(sig[k] >= 0.0f) || isinf(sig[k])) return fail(RTW_EINVAL, "%s must be finite and >= 0", names[k]);
  return RTW_OK;
}

// rtw_denoise's loops; `count` (or NULL) is rtw_denoise_counts' per-pixel sample count, which replaces n
int denoise_host(const float* sum, const float* sq, const float* albedo, const float* normal, const float* depth,
                 const float* count, uint32_t w, uint32_t h, uint32_t samples, const uint32_t* tile_samples,
                 uint32_t iterations, float sigma_l, float sigma_n, float sigma_z, float* out);

}  // namespace

extern "C" {

int rtw_denoise_scratch_bytes(uint32_t w, uint32_t h, uint64_t* bytes) {
  if (!bytes) return fail(RTW_EINVAL, "NULL argument");
  if (int e = check_image_min(w, h)) return e;
  if (int e = check_image_max(w, h)) return e;
  *bytes = (uint64_t)w * h * DENOISE_SCRATCH_PER_PIXEL;
  return RTW_OK;
}

int rtw_denoise_device(int device, const float* d_sum, const float* d_sq, const float* d_albedo, const float* d_normal,
                       const float* d_depth, uint32_t w, uint32_t h, uint32_t samples, const uint32_t* d_tile_samples,
                       uint32_t iterations, float sigma_l, float sigma_n, float sigma_z, float* d_out, void* d_scratch,
                       void* stream) {
  if (int e = check_denoise(d_sum, d_out, d_scratch != nullptr, w, h, samples, d_tile_samples, iterations, sigma_l,
                            sigma_n, sigma_z))
    return e;
  if ((uintptr_t)d_scratch & 15u) return fail(RTW_EINVAL, "d_scratch must be 16-byte aligned");
  DeviceGuard g;
  if (device >= 0) HIPCHK(hipSetDevice(device), "hipSetDevice");
  return enqueue_denoise(d_sum, d_sq, d_albedo, d_normal, d_depth, nullptr, w, h, samples, d_tile_samples, iterations,
                         sigma_l, sigma_n, sigma_z, d_out, d_scratch, abi_stream(stream));
}

int rtw_denoise_counts_device(int device, const float* d_sum, const float* d_sq, const float* d_albedo,
                              const float* d_normal, const float* d_depth, const float* d_count, uint32_t w,
                              uint32_t h, uint32_t iterations, float sigma_l, float sigma_n, float sigma_z,
                              float* d_out, void* d_scratch, void* stream) {
  // (the shared checks with count among the first one's buffers and a `samples` that passes)
  if (int e = check_denoise(d_count ? d_sum : nullptr, d_out, d_scratch != nullptr, w, h, 1, nullptr, iterations,
                            sigma_l, sigma_n, sigma_z))
    return e;
  if ((uintptr_t)d_scratch & 15u) return fail(RTW_EINVAL, "d_scratch must be 16-byte aligned");
  DeviceGuard g;
  if (device >= 0) HIPCHK(hipSetDevice(device), "hipSetDevice");
  return enqueue_denoise(d_sum, d_sq, d_albedo, d_normal, d_depth, d_count, w, h, 0, nullptr, iterations, sigma_l,
                         sigma_n, sigma_z, d_out, d_scratch, abi_stream(stream));
}

int rtw_denoise_counts(const float* sum, const float* sq, const float* albedo, const float* normal, const float* depth,
                       const float* count, uint32_t w, uint32_t h, uint32_t iterations, float sigma_l, float sigma_n,
                       float sigma_z, float* out) {
  if (int e = check_denoise(count ? sum : nullptr, out, true, w, h, 1, nullptr, iterations, sigma_l, sigma_n, sigma_z))
    return e;
  return denoise_host(sum, sq, albedo, normal, depth, count, w, h, 0, nullptr, iterations, sigma_l, sigma_n, sigma_z,
                      out);
}

int rtw_denoise(const float* sum, const float* sq, const float* albedo, const float* normal, const float* depth,
                uint32_t w, uint32_t h, uint32_t samples, const uint32_t* tile_samples, uint32_t iterations,
                float sigma_l, float sigma_n, float sigma_z, float* out) {
  if (int e = check_denoise(sum, out, true, w, h, samples, tile_samples, iterations, sigma_l, sigma_n, sigma_z))
    return e;
  return denoise_host(sum, sq, albedo, normal, depth, nullptr, w, h, samples, tile_samples, iterations, sigma_l,
                      sigma_n, sigma_z, out);
}

}  // extern "C"

namespace {

int denoise_host(const float* sum, const float* sq, const float* albedo, const float* normal, const float* depth,
                 const float* count, uint32_t w, uint32_t h, uint32_t samples, const uint32_t* tile_samples,
                 uint32_t iterations, float sigma_l, float sigma_n, float sigma_z, float* out) {
  const size_t px = (size_t)w * h;
  const uint32_t tiles_x = (w + 7u) / 8u;
  std::vector<Rec> X, Y;
  std::vector<Guide> G;
  std::vector<float> D;
  std::vector<uint8_t> live;
  try {
    X.resize(px), Y.resize(px), G.resize(px), D.resize(px * 3), live.resize(px);
  } catch (const std::bad_alloc&) {
    return fail(RTW_ENOMEM, "rtw_denoise: no memory for a %ux%u frame", w, h);
  }
  // prepare
  for (uint32_t row = 0; row < h; ++row)
    for (uint32_t i = 0; i < w; ++i) {
      const size_t p = (size_t)row * w + i;
      const uint32_t n = tile_samples ? tile_samples[(size_t)(row >> 3) * tiles_x + (i >> 3)] : samples;
      Rec& r = X[p];
      Guide& g = G[p];
      g = Guide{{0.0f, 0.0f, 0.0f}, 0.0f};
      const bool empty = count ? !(count[p] > 0.0f) : n == 0;  // (a NaN count is empty)
      live[p] = !empty;
      if (empty) {
        const uint32_t bits = 0x7FC00000u;
        float nan;
        memcpy(&nan, &bits, 4);
        r = Rec{{nan, nan, nan}, 0.0f};
        D[p * 3] = D[p * 3 + 1] = D[p * 3 + 2] = 1.0f;
        continue;
      }
      const float inv = 1.0f / (count ? count[p] : (float)n);
      float m[3], d[3];
      for (int c = 0; c < 3; ++c) {
        m[c] = sum[p * 3 + c] * inv;
        d[c] = 1.0f;
        if (albedo) {
          const float a = albedo[p * 3 + c] * inv;
          d[c] = a > 0.001f ? a : 0.001f;
        }
        r.x[c] = m[c] / d[c];
        D[p * 3 + c] = d[c];
      }
      r.var = 0.0f;
      if (sq) {
        float u[3];
        for (int c = 0; c < 3; ++c) {
          float v = sq[p * 3 + c] * inv - m[c] * m[c];
          v = v < 0.0f ? 0.0f : v;  // tile_noise_kernel's clamp: a NaN stays
          u[c] = (v * inv) / (d[c] * d[c]);
        }
        r.var = (u[0] + u[1]) + u[2];
      }
      if (normal) {
        const float* nr = normal + p * 3;
        const float nn = (nr[0] * nr[0] + nr[1] * nr[1]) + nr[2] * nr[2];
        if (nn > 0.0f) {
          const float len = sqrtf(nn);
          for (int c = 0; c < 3; ++c) g.g[c] = nr[c] / len;
        }
      }
      if (depth) g.z = depth[p * 2] * inv;
    }
  // iterations
  static const float H[3] = {0.375f, 0.25f, 0.0625f};
  const bool use_n = sigma_n != 0.0f, use_z = sigma_z != 0.0f, use_l = sigma_l != 0.0f && sq;
  const float k_n = use_n ? 1.0f / (sigma_n * sigma_n) : 0.0f;
  for (uint32_t k = 0; k < iterations; ++k) {
    const int64_t step = (int64_t)1 << k;
    const float sz_step = sigma_z * (float)step;
    for (int64_t row = 0; row < (int64_t)h; ++row)
      for (int64_t i = 0; i < (int64_t)w; ++i) {
        const size_t p = (size_t)row * w + (size_t)i;
        const Rec& xp = X[p];
        const Guide& gp = G[p];
        const float l_p = lum(xp);
        const float rz = 1.0f / (sz_step * fabsf(gp.z) + 1e-6f);
        const float rl = 1.0f / (sigma_l * sqrtf(xp.var) + 1e-4f);
        float sw = 0.0f, sx[3] = {0.0f, 0.0f, 0.0f}, sv = 0.0f;
        for (int dy = -2; dy <= 2; ++dy) {
          const int64_t qy = row + dy * step;
          if (qy < 0 || qy >= (int64_t)h) continue;
          for (int dx = -2; dx <= 2; ++dx) {
            const int64_t qx = i + dx * step;
            if (qx < 0 || qx >= (int64_t)w) continue;
            const size_t q = (size_t)qy * w + (size_t)qx;
            const Rec& xq = X[q];
            const Guide& gq = G[q];
            float wt = H[dx < 0 ? -dx : dx] * H[dy < 0 ? -dy : dy];
            if (use_n) {
              const float e0 = gp.g[0] - gq.g[0], e1 = gp.g[1] - gq.g[1], e2 = gp.g[2] - gq.g[2];
              const float dn2 = (e0 * e0 + e1 * e1) + e2 * e2;
              wt = wt * max0(1.0f - dn2 * k_n);
            }
            if (use_z) wt = wt * max0(1.0f - fabsf(gp.z - gq.z) * rz);
            const float l_q = lum(xq);
            if (use_l) wt = wt * max0(1.0f - fabsf(l_p - l_q) * rl);
            if (wt > 0.0f && l_q == l_q) {
              sw = sw + wt;
              for (int c = 0; c < 3; ++c) sx[c] = sx[c] + wt * xq.x[c];
              sv = sv + (wt * wt) * xq.var;
            }
          }
        }
        Rec r = xp;
        if (sw > 0.0f) r = Rec{{sx[0] / sw, sx[1] / sw, sx[2] / sw}, sv / (sw * sw)};
        Y[p] = r;
      }
    std::swap(X, Y);
  }
  // finish
  for (size_t p = 0; p < px; ++p)
    for (int c = 0; c < 3; ++c) out[p * 3 + c] = live[p] ? X[p].x[c] * D[p * 3 + c] : 0.0f;
  return RTW_OK;
}

}  // namespace
