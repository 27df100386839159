// rtw_temporal_kernel.hpp — temporal accumulation behind rtw_temporal_device (include/rtw.h states the arithmetic
// operation by operation; DESIGN.md §4 "Temporal accumulation" the rationale and the measurements).  One kernel over the
// full w x h layout, one thread per pixel, all f32 with one rounding per operation (-ffp-contract=off), IEEE division,
// sqrt and floorf, no transcendentals, plain vector loads and stores, no atomics, no LDS:
//   temporal_kernel   the current frame's five sums (14 floats per pixel), reprojected through its mean first-hit depth
//                     into the history camera; up to four bilinear taps of the history's six buffers (15 floats each);
//                     the six outputs (15 floats).
// A workgroup is 256 threads = 32 x 8 pixels as the denoiser's, a wave two rows of 32: a wave's loads and stores of a
// 3-float buffer are two runs of 384 contiguous bytes, 12 bytes per lane.  The taps' addresses depend on the data; for
// about a pixel of camera motion neighbouring lanes gather neighbouring history pixels, and L2 serves the 4-fold reuse.
// A pixel loads in three rounds, each issued as a whole before its first use, so that at most three memory latencies
// are exposed per pixel: its own 14 floats; every buffer of all four taps (the addresses clamped onto the image, so
// that no load waits for a test; a tap off the image or failing a test is loaded and not counted); then it stores.
// No store comes before the last load, so an out buffer may be its own current-frame buffer.  Included by
// rtw_kernel.hip alone.
#pragma once
#include "rtw_dev_math.hpp"

namespace rtw {
namespace dev {

constexpr int TEMPORAL_TX = 32, TEMPORAL_TY = 8, TEMPORAL_BLOCK = TEMPORAL_TX * TEMPORAL_TY;
// the five buffers' channels and where each begins among a pixel's 14 floats: sum, sq, albedo, normal, depth
constexpr int TEMPORAL_CH[5] = {3, 3, 3, 3, 2};
constexpr int TEMPORAL_AT[5] = {0, 3, 6, 9, 12};

__device__ __forceinline__ float temporal_dot(const float* a, const float* b) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
// a pixel's `ch` floats of one buffer (one load of 12 or 8 bytes per lane), or +0 for a buffer out of use
__device__ __forceinline__ void temporal_load(const float* buf, size_t pixel, int ch, float* v) {
  v[0] = v[1] = 0.0f;
  if (ch == 3) v[2] = 0.0f;
  if (!buf) return;
  const float* s = buf + pixel * (size_t)ch;
  v[0] = s[0];
  v[1] = s[1];
  if (ch == 3) v[2] = s[2];
}
// the unit normal of a normal sum as denoise_prepare_kernel makes it: +0 for a zero sum
__device__ __forceinline__ void temporal_unit(const float* n, float* g) {
  const float nn = temporal_dot(n, n);
  g[0] = g[1] = g[2] = 0.0f;
  if (nn > 0.0f) {
    const float len = sqrtf(nn);
    g[0] = n[0] / len;
    g[1] = n[1] / len;
    g[2] = n[2] / len;
  }
}

__global__ __launch_bounds__(TEMPORAL_BLOCK) void temporal_kernel(TemporalArgs a) {
  const uint32_t i = blockIdx.x * TEMPORAL_TX + (threadIdx.x & (TEMPORAL_TX - 1));
  const uint32_t row = blockIdx.y * TEMPORAL_TY + threadIdx.x / TEMPORAL_TX;
  if (i >= a.w || row >= a.h) return;
  const size_t p = (size_t)row * a.w + i;
  const float* curp[5] = {a.sum, a.sq, a.albedo, a.normal, a.depth};
  const float* histp[5] = {a.hist_sum, a.hist_sq, a.hist_albedo, a.hist_normal, a.hist_depth};
  float* outp[5] = {a.out_sum, a.out_sq, a.out_albedo, a.out_normal, a.out_depth};
  const uint32_t n = a.tile_samples ? a.tile_samples[(size_t)(row >> 3) * a.tiles_x + (i >> 3)] : a.samples;
  if (n == 0u) {  // an empty pixel: every output +0
#pragma unroll
    for (int f = 0; f < 5; ++f)
      if (outp[f])
        for (int c = 0; c < TEMPORAL_CH[f]; ++c) outp[f][p * TEMPORAL_CH[f] + c] = 0.0f;
    a.out_count[p] = 0.0f;
    return;
  }
  const float c_cur = (float)n;
  // round 1: the pixel's own values (a buffer out of use stays +0 and is never stored)
  float X[14];
#pragma unroll
  for (int f = 0; f < 5; ++f)
    temporal_load(curp[f], p, TEMPORAL_CH[f], X + TEMPORAL_AT[f]);
  float out_count = c_cur;
  const float hits = X[13];
  if (a.hist_count && hits > 0.0f) {
    const rtw_camera& cc = a.cam;
    const rtw_camera& hc = a.hist_cam;
    const float w1 = (float)(a.w - 1u), h1 = (float)(a.h - 1u);
    const float tbar = X[12] / hits;
    const uint32_t j = a.h - 1u - row;
    const float s = ((float)i + 0.5f) / w1, v = ((float)j + 0.5f) / h1;
    float r[3], e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float d = ((cc.lower_left_corner[k] + s * cc.horizontal[k]) + v * cc.vertical[k]) - cc.origin[k];
      const float P = cc.origin[k] + tbar * d;
      r[k] = P - hc.origin[k];
      e[k] = hc.lower_left_corner[k] - hc.origin[k];
    }
    const float tau = temporal_dot(r, hc.w) / temporal_dot(e, hc.w);
    const float s2 = (temporal_dot(r, hc.horizontal) / tau - temporal_dot(e, hc.horizontal)) /
                     temporal_dot(hc.horizontal, hc.horizontal);
    const float v2 = (temporal_dot(r, hc.vertical) / tau - temporal_dot(e, hc.vertical)) /
                     temporal_dot(hc.vertical, hc.vertical);
    const float x = s2 * w1 - 0.5f;
    const float y = h1 - (v2 * h1 - 0.5f);
    if (tau > 0.0f && x >= -1.0f && x < (float)a.w && y >= -1.0f && y < (float)a.h) {  // (a NaN fails)
      const float x0 = floorf(x), y0 = floorf(y);
      const float fx = x - x0, fy = y - y0, gx = 1.0f - fx, gy = 1.0f - fy;
      const int ix = (int)x0, iy = (int)y0;  // -1 .. w - 1 and -1 .. h - 1: sides <= 65536
      const int wi = (int)a.w, hi = (int)a.h;
      const float b[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
      // round 2: all four taps' 15 floats, the addresses clamped onto the image
      float T[4][14], L[4];
      bool on[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int qx = ix + (t & 1), qy = iy + (t >> 1);
        on[t] = qx >= 0 && qx < wi && qy >= 0 && qy < hi;
        const int cx = qx < 0 ? 0 : (qx >= wi ? wi - 1 : qx), cy = qy < 0 ? 0 : (qy >= hi ? hi - 1 : qy);
        const size_t q = (size_t)cy * a.w + (size_t)cx;
        L[t] = a.hist_count[q];
#pragma unroll
        for (int f = 0; f < 5; ++f)
          temporal_load(histp[f], q, TEMPORAL_CH[f], T[t] + TEMPORAL_AT[f]);
      }
      float gp[3];
      temporal_unit(X + 9, gp);
      float sb = 0.0f, sL = 0.0f, S[14];
#pragma unroll
      for (int k = 0; k < 14; ++k) S[k] = 0.0f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {  // in tap order: the order is the contract
        bool cnt = on[t] && b[t] > 0.0f && L[t] > 0.0f && T[t][13] > 0.0f;
        const float zq = T[t][12] / T[t][13];
        cnt = cnt && fabsf(tau - zq) <= a.tol_z * tau;
        if (a.normal) {
          float gq[3];
          temporal_unit(T[t] + 9, gq);
          cnt = cnt && temporal_dot(gp, gq) >= a.cos_n;
        }
        const float fin = (T[t][0] + T[t][1]) + T[t][2];
        cnt = cnt && fin - fin == 0.0f;
        if (cnt) {
          sb = sb + b[t];
          sL = sL + b[t] * L[t];
#pragma unroll
          for (int k = 0; k < 14; ++k) S[k] = S[k] + b[t] * T[t][k];
        }
      }
      if (sb > 0.0f) {
        const float Lr = sL / sb;
        const float lam = Lr > a.max_history ? a.max_history / Lr : 1.0f;
        const float k_h = lam / sb;
#pragma unroll
        for (int k = 0; k < 14; ++k) X[k] = X[k] + k_h * S[k];
        out_count = c_cur + k_h * sL;
      }
    }
  }
  // round 3: the outputs
#pragma unroll
  for (int f = 0; f < 5; ++f)
    if (outp[f]) {
#pragma unroll
      for (int c = 0; c < TEMPORAL_CH[f]; ++c) outp[f][p * TEMPORAL_CH[f] + c] = X[TEMPORAL_AT[f] + c];
    }
  a.out_count[p] = out_count;
}

}  // namespace dev
}  // namespace rtw
