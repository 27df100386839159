// rtw_temporal.cpp — temporal accumulation's C-ABI calls (include/rtw.h): rtw_temporal_device (checks, then
// rtw_kernel.hip's enqueue_temporal) and rtw_temporal, the same arithmetic as plain loops over host arrays: what
// rtw_denoise is beside rtw_denoise_device.  The operation is defined in the header operation by operation; this file
// and rtw_temporal_kernel.hpp restate it independently and agree bit for bit (-ffp-contract=off, IEEE division, sqrt
// and floorf; tests/test_temporal_abi.py holds this one to a numpy restatement, tests/test_gpu_temporal.py the kernel
// to both).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/rtw.h"
#include "rtw_scene.hpp"

using namespace rtw;

namespace {

inline float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the checks both calls share, in the header's order; the arguments as TemporalArgs holds them
int check_temporal(const TemporalArgs& a, const rtw_camera* cam, const rtw_camera* hist_cam) {
  if (!a.sum || !a.depth || !cam || !a.out_sum || !a.out_depth || !a.out_count) return fail(RTW_EINVAL, "NULL buffer");
  const void* cur[3] = {a.sq, a.albedo, a.normal};
  const void* out[3] = {a.out_sq, a.out_albedo, a.out_normal};
  const void* hist[3] = {a.hist_sq, a.hist_albedo, a.hist_normal};
  const char* names[3] = {"sq", "albedo", "normal"};
  for (int k = 0; k < 3; ++k)
    if (!cur[k] != !out[k]) return fail(RTW_EINVAL, "%s: the current and the out buffer are both given or both NULL", names[k]);
  if (a.hist_count) {
    if (!a.hist_sum || !a.hist_depth || !hist_cam) return fail(RTW_EINVAL, "NULL history buffer");
    for (int k = 0; k < 3; ++k)
      if (cur[k] && !hist[k]) return fail(RTW_EINVAL, "NULL history buffer: hist_%s, whose triple is in use", names[k]);
    const void* outs[6] = {a.out_sum, a.out_sq, a.out_albedo, a.out_normal, a.out_depth, a.out_count};
    const void* hists[6] = {a.hist_sum, a.hist_sq, a.hist_albedo, a.hist_normal, a.hist_depth, a.hist_count};
    for (const void* o : outs)
      for (const void* q : hists)
        if (o && o == q) return fail(RTW_EINVAL, "an out buffer is a history buffer: the call gathers");
  }
  if (int e = check_image_min(a.w, a.h)) return e;
  if (int e = check_image_max(a.w, a.h)) return e;
  if (a.samples == 0 && !a.tile_samples) return fail(RTW_EINVAL, "samples must be > 0 without a tile table");
  if (!(a.max_history >= 0.0f) || isinf(a.max_history)) return fail(RTW_EINVAL, "max_history must be finite and >= 0");
  if (!(a.tol_z >= 0.0f) || isinf(a.tol_z)) return fail(RTW_EINVAL, "tol_z must be finite and >= 0");
  if (!(a.cos_n >= -1.0f && a.cos_n <= 1.0f)) return fail(RTW_EINVAL, "cos_n must be within [-1, 1]");
  return RTW_OK;
}

TemporalArgs pack(const float* sum, const float* sq, const float* albedo, const float* normal, const float* depth,
                  uint32_t w, uint32_t h, uint32_t samples, const uint32_t* tile_samples, const rtw_camera* cam,
                  const float* hist_sum, const float* hist_sq, const float* hist_albedo, const float* hist_normal,
                  const float* hist_depth, const float* hist_count, const rtw_camera* hist_cam, float max_history,
                  float tol_z, float cos_n, float* out_sum, float* out_sq, float* out_albedo, float* out_normal,
                  float* out_depth, float* out_count) {
  TemporalArgs a;
  memset(&a, 0, sizeof a);
  a.sum = sum; a.sq = sq; a.albedo = albedo; a.normal = normal; a.depth = depth;
  a.tile_samples = tile_samples;
  a.hist_sum = hist_sum; a.hist_sq = hist_sq; a.hist_albedo = hist_albedo; a.hist_normal = hist_normal;
  a.hist_depth = hist_depth; a.hist_count = hist_count;
  a.out_sum = out_sum; a.out_sq = out_sq; a.out_albedo = out_albedo; a.out_normal = out_normal;
  a.out_depth = out_depth; a.out_count = out_count;
  a.w = w; a.h = h; a.tiles_x = (w + 7u) / 8u; a.samples = samples;
  a.max_history = max_history; a.tol_z = tol_z; a.cos_n = cos_n;
  if (cam) a.cam = *cam;
  if (hist_cam && hist_count) a.hist_cam = *hist_cam;
  return a;
}

// after the checks: a triple out of use is NULL in all three places, and without a history every hist pointer is
inline void drop_unused(TemporalArgs& a) {
  if (!a.sq) a.hist_sq = nullptr;
  if (!a.albedo) a.hist_albedo = nullptr;
  if (!a.normal) a.hist_normal = nullptr;
  if (!a.hist_count) a.hist_sum = a.hist_sq = a.hist_albedo = a.hist_normal = a.hist_depth = nullptr;
}

// one buffer's share of a pixel: out = cur + k * (the taps' weighted sum), or cur alone (use = false), or +0
template <int CH>
inline void emit(const float* cur, const float* hist, float* out, size_t p, const size_t* q, const float* b, int n_taps,
                 bool empty, bool use, float k) {
  if (!cur) return;
  for (int c = 0; c < CH; ++c) {
    float v = empty ? 0.0f : cur[p * CH + c];
    if (use) {
      float s = 0.0f;
      for (int t = 0; t < n_taps; ++t) s = s + b[t] * hist[q[t] * CH + c];
      v = v + k * s;
    }
    out[p * CH + c] = v;
  }
}

}  // namespace

extern "C" {

int rtw_temporal_device(int device, const float* d_sum, const float* d_sq, const float* d_albedo, const float* d_normal,
                        const float* d_depth, uint32_t w, uint32_t h, uint32_t samples, const uint32_t* d_tile_samples,
                        const rtw_camera* cam, const float* d_hist_sum, const float* d_hist_sq,
                        const float* d_hist_albedo, const float* d_hist_normal, const float* d_hist_depth,
                        const float* d_hist_count, const rtw_camera* hist_cam, float max_history, float tol_z,
                        float cos_n, float* d_out_sum, float* d_out_sq, float* d_out_albedo, float* d_out_normal,
                        float* d_out_depth, float* d_out_count, void* stream) {
  TemporalArgs a = pack(d_sum, d_sq, d_albedo, d_normal, d_depth, w, h, samples, d_tile_samples, cam, d_hist_sum,
                        d_hist_sq, d_hist_albedo, d_hist_normal, d_hist_depth, d_hist_count, hist_cam, max_history,
                        tol_z, cos_n, d_out_sum, d_out_sq, d_out_albedo, d_out_normal, d_out_depth, d_out_count);
  if (int e = check_temporal(a, cam, hist_cam)) return e;
  drop_unused(a);
  DeviceGuard g;
  if (device >= 0) HIPCHK(hipSetDevice(device), "hipSetDevice");
  return enqueue_temporal(a, abi_stream(stream));
}

int rtw_temporal(const float* sum, const float* sq, const float* albedo, const float* normal, const float* depth,
                 uint32_t w, uint32_t h, uint32_t samples, const uint32_t* tile_samples, const rtw_camera* cam,
                 const float* hist_sum, const float* hist_sq, const float* hist_albedo, const float* hist_normal,
                 const float* hist_depth, const float* hist_count, const rtw_camera* hist_cam, float max_history,
                 float tol_z, float cos_n, float* out_sum, float* out_sq, float* out_albedo, float* out_normal,
                 float* out_depth, float* out_count) {
  TemporalArgs a = pack(sum, sq, albedo, normal, depth, w, h, samples, tile_samples, cam, hist_sum, hist_sq,
                        hist_albedo, hist_normal, hist_depth, hist_count, hist_cam, max_history, tol_z, cos_n, out_sum,
                        out_sq, out_albedo, out_normal, out_depth, out_count);
  if (int e = check_temporal(a, cam, hist_cam)) return e;
  drop_unused(a);
  const rtw_camera &cc = a.cam, &hc = a.hist_cam;
  const float wf = (float)w, hf = (float)h, w1 = (float)(w - 1u), h1 = (float)(h - 1u);
  for (uint32_t row = 0; row < h; ++row)
    for (uint32_t i = 0; i < w; ++i) {
      const size_t p = (size_t)row * w + i;
      const uint32_t n = tile_samples ? tile_samples[(size_t)(row >> 3) * a.tiles_x + (i >> 3)] : samples;
      const bool empty = n == 0;
      const float c = (float)n;
      size_t q[4];
      float b[4];
      int n_taps = 0;
      float sb = 0.0f, sL = 0.0f;
      const float hits = depth[p * 2 + 1];
      if (!empty && a.hist_count && hits > 0.0f) {
        const float tbar = depth[p * 2] / hits;
        const uint32_t j = h - 1u - row;
        const float s = ((float)i + 0.5f) / w1, v = ((float)j + 0.5f) / h1;
        float r[3], e[3];
        for (int k = 0; k < 3; ++k) {
          const float d = ((cc.lower_left_corner[k] + s * cc.horizontal[k]) + v * cc.vertical[k]) - cc.origin[k];
          const float P = cc.origin[k] + tbar * d;
          r[k] = P - hc.origin[k];
          e[k] = hc.lower_left_corner[k] - hc.origin[k];
        }
        const float tau = dot3(r, hc.w) / dot3(e, hc.w);
        const float s2 = (dot3(r, hc.horizontal) / tau - dot3(e, hc.horizontal)) / dot3(hc.horizontal, hc.horizontal);
        const float v2 = (dot3(r, hc.vertical) / tau - dot3(e, hc.vertical)) / dot3(hc.vertical, hc.vertical);
        const float x = s2 * w1 - 0.5f;
        const float y = h1 - (v2 * h1 - 0.5f);
        if (tau > 0.0f && x >= -1.0f && x < wf && y >= -1.0f && y < hf) {
          const float x0 = floorf(x), y0 = floorf(y);
          const float fx = x - x0, fy = y - y0, gx = 1.0f - fx, gy = 1.0f - fy;
          const int64_t ix = (int64_t)x0, iy = (int64_t)y0;  // -1 .. w - 1, -1 .. h - 1
          const float bw[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
          float gp[3] = {0.0f, 0.0f, 0.0f};
          if (normal) {
            const float* nr = normal + p * 3;
            const float nn = dot3(nr, nr);
            if (nn > 0.0f) {
              const float len = sqrtf(nn);
              for (int k = 0; k < 3; ++k) gp[k] = nr[k] / len;
            }
          }
          for (int t = 0; t < 4; ++t) {
            const int64_t qx = ix + (t & 1), qy = iy + (t >> 1);
            if (qx < 0 || qx >= (int64_t)w || qy < 0 || qy >= (int64_t)h) continue;
            if (!(bw[t] > 0.0f)) continue;
            const size_t qq = (size_t)qy * w + (size_t)qx;
            const float Lq = a.hist_count[qq];
            if (!(Lq > 0.0f)) continue;
            const float hq = a.hist_depth[qq * 2 + 1];
            if (!(hq > 0.0f)) continue;
            const float zq = a.hist_depth[qq * 2] / hq;
            if (!(fabsf(tau - zq) <= tol_z * tau)) continue;
            if (normal) {
              const float* nq = a.hist_normal + qq * 3;
              float gq[3] = {0.0f, 0.0f, 0.0f};
              const float nn = dot3(nq, nq);
              if (nn > 0.0f) {
                const float len = sqrtf(nn);
                for (int k = 0; k < 3; ++k) gq[k] = nq[k] / len;
              }
              if (!(dot3(gp, gq) >= cos_n)) continue;
            }
            const float* sq3 = a.hist_sum + qq * 3;
            const float fin = (sq3[0] + sq3[1]) + sq3[2];
            if (!(fin - fin == 0.0f)) continue;
            q[n_taps] = qq;
            b[n_taps] = bw[t];
            ++n_taps;
            sb = sb + bw[t];
            sL = sL + bw[t] * Lq;
          }
        }
      }
      const bool use = sb > 0.0f;
      float k = 0.0f;
      if (use) {
        const float Lr = sL / sb;
        const float lam = Lr > max_history ? max_history / Lr : 1.0f;
        k = lam / sb;
      }
      emit<3>(sum, a.hist_sum, out_sum, p, q, b, n_taps, empty, use, k);
      emit<3>(sq, a.hist_sq, out_sq, p, q, b, n_taps, empty, use, k);
      emit<3>(albedo, a.hist_albedo, out_albedo, p, q, b, n_taps, empty, use, k);
      emit<3>(normal, a.hist_normal, out_normal, p, q, b, n_taps, empty, use, k);
      emit<2>(depth, a.hist_depth, out_depth, p, q, b, n_taps, empty, use, k);
      out_count[p] = empty ? 0.0f : (use ? c + k * sL : c);
    }
  return RTW_OK;
}

}  // extern "C"
