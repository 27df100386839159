// rtw_denoise_kernel.hpp — the edge-avoiding à-trous wavelet filter behind rtw_denoise_device (include/rtw.h states
// the arithmetic operation by operation; DESIGN.md §4 "Denoiser" the mapping and the measurements).  Three kernels over
// the full w x h layout, all f32 with one rounding per operation (-ffp-contract=off), IEEE division and sqrt, no
// transcendentals, plain vector loads and stores, no atomics:
//   denoise_prepare_kernel  the five sums -> per pixel three 16-byte records in the call's scratch: X = (x_0, x_1, x_2,
//                           var), the albedo-demodulated mean and the variance of its mean; G = (g_0, g_1, g_2, z), the
//                           unit normal and the mean depth; D = (d_0, d_1, d_2, live), the albedo the finish multiplies
//                           back and 1.0f / +0 for a pixel with / without samples;
//   denoise_atrous_kernel   one iteration: X, G -> X' (48 bytes of traffic per pixel), or with FIN the finish in its
//                           place: X, G, D -> out.  LDS: the workgroup's 32 x 8 pixels and their halo of 2 * step come
//                           through an LDS tile of X and G records; otherwise every tap is a global load (L1 / L2 serve
//                           the 25-fold reuse).  Both forms add the taps in the contract's order -- dy outer, dx inner --
//                           through one body, so they agree bit for bit;
//   denoise_finish_kernel   X, D -> out for iterations = 0.
// A workgroup is 256 threads = 32 x 8 pixels, a wave two rows of 32: a wave's X or G loads and stores are two runs of
// 512 contiguous bytes, 16 bytes per lane.  Included by rtw_kernel.hip alone.
#pragma once
#include "rtw_dev_math.hpp"

namespace rtw {
namespace dev {

constexpr int DENOISE_TX = 32, DENOISE_TY = 8, DENOISE_BLOCK = DENOISE_TX * DENOISE_TY;

struct DenoiseArgs {
  const float* sum;     // 3 floats per pixel
  const float* sq;      // 3, or NULL
  const float* albedo;  // 3, or NULL
  const float* normal;  // 3, or NULL
  const float* depth;   // 2, or NULL
  const uint32_t* tile_samples;  // per 8x8 tile, or NULL: `samples` everywhere
  const float* count;   // 1 float per pixel (rtw_denoise_counts_device: it replaces n), or NULL
  uint32_t w, h, tiles_x, samples;
  float4* X;  // scratch: the iteration's input records
  float4* Y;  // scratch: its output records
  float4* G;
  float4* D;
  float* out;  // 3 floats per pixel
  // one iteration
  uint32_t step;
  float k_n;      // 1 / sigma_n^2, the host's
  float sz_step;  // sigma_z * (float)step, the host's
  float sigma_l;
  uint32_t use_n, use_z, use_l;  // a sigma of 0 (and for use_l a NULL sq) drops its factor
};

__device__ __forceinline__ float max0(float v) { return v > 0.0f ? v : 0.0f; }  // a NaN gives 0
__device__ __forceinline__ float denoise_lum(const float4& x) {
  return (0.2126f * x.x + 0.7152f * x.y) + 0.0722f * x.z;
}

__global__ __launch_bounds__(DENOISE_BLOCK) void denoise_prepare_kernel(DenoiseArgs a) {
  const uint32_t i = blockIdx.x * DENOISE_TX + (threadIdx.x & (DENOISE_TX - 1));
  const uint32_t row = blockIdx.y * DENOISE_TY + threadIdx.x / DENOISE_TX;
  if (i >= a.w || row >= a.h) return;
  const size_t p = (size_t)row * a.w + i;
  const uint32_t n = a.tile_samples ? a.tile_samples[(size_t)(row >> 3) * a.tiles_x + (i >> 3)] : a.samples;
  const float cnt = a.count ? a.count[p] : (float)n;
  if (a.count ? !(cnt > 0.0f) : n == 0u) {  // an empty pixel: never a tap (its luminance is a NaN), output +0
    const float nan = __uint_as_float(0x7FC00000u);
    a.X[p] = make_float4(nan, nan, nan, 0.0f);
    a.D[p] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    a.G[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const float inv = 1.0f / cnt;
  const float* s = a.sum + p * 3u;
  const float m0 = s[0] * inv, m1 = s[1] * inv, m2 = s[2] * inv;
  float d0 = 1.0f, d1 = 1.0f, d2 = 1.0f;
  if (a.albedo) {
    const float* al = a.albedo + p * 3u;
    const float a0 = al[0] * inv, a1 = al[1] * inv, a2 = al[2] * inv;
    d0 = a0 > 0.001f ? a0 : 0.001f;
    d1 = a1 > 0.001f ? a1 : 0.001f;
    d2 = a2 > 0.001f ? a2 : 0.001f;
  }
  float var = 0.0f;
  if (a.sq) {
    const float* q = a.sq + p * 3u;
    float v0 = q[0] * inv - m0 * m0, v1 = q[1] * inv - m1 * m1, v2 = q[2] * inv - m2 * m2;
    v0 = v0 < 0.0f ? 0.0f : v0;  // tile_noise_kernel's clamp: a NaN stays
    v1 = v1 < 0.0f ? 0.0f : v1;
    v2 = v2 < 0.0f ? 0.0f : v2;
    const float u0 = (v0 * inv) / (d0 * d0), u1 = (v1 * inv) / (d1 * d1), u2 = (v2 * inv) / (d2 * d2);
    var = (u0 + u1) + u2;
  }
  float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, z = 0.0f;
  if (a.normal) {
    const float* nr = a.normal + p * 3u;
    const float n0 = nr[0], n1 = nr[1], n2 = nr[2];
    const float nn = (n0 * n0 + n1 * n1) + n2 * n2;
    if (nn > 0.0f) {
      const float len = sqrtf(nn);
      g0 = n0 / len;
      g1 = n1 / len;
      g2 = n2 / len;
    }
  }
  if (a.depth) z = a.depth[p * 2u] * inv;
  a.X[p] = make_float4(m0 / d0, m1 / d1, m2 / d2, var);
  a.G[p] = make_float4(g0, g1, g2, z);
  a.D[p] = make_float4(d0, d1, d2, 1.0f);
}

__global__ __launch_bounds__(DENOISE_BLOCK) void denoise_finish_kernel(DenoiseArgs a) {
  const uint32_t i = blockIdx.x * DENOISE_TX + (threadIdx.x & (DENOISE_TX - 1));
  const uint32_t row = blockIdx.y * DENOISE_TY + threadIdx.x / DENOISE_TX;
  if (i >= a.w || row >= a.h) return;
  const size_t p = (size_t)row * a.w + i;
  const float4 x = a.X[p], d = a.D[p];
  float* o = a.out + p * 3u;
  const bool live = d.w != 0.0f;
  o[0] = live ? x.x * d.x : 0.0f;
  o[1] = live ? x.y * d.y : 0.0f;
  o[2] = live ? x.z * d.z : 0.0f;
}

// One iteration for the pixel (i, row) = blockIdx * (32, 8) + the thread's place in the workgroup.  The LDS form's tile
// is (32 + 4 step) x (8 + 4 step) records of X, then as many of G, filled row by row by the whole workgroup (16 bytes
// per lane, consecutive lanes consecutive records); records off the image are not filled and never read, since taps
// off the image are skipped in both forms.  Consecutive lanes read consecutive 16-byte records, so every ds_read_b128
// lane group covers 16 different slots of the bank row whatever the tile's width.
template <bool LDS, bool FIN>
__global__ __launch_bounds__(DENOISE_BLOCK) void denoise_atrous_kernel(DenoiseArgs a) {
  extern __shared__ __attribute__((aligned(16))) float4 denoise_tile[];
  const int step = (int)a.step, halo = 2 * step;
  const int lx = (int)(threadIdx.x & (DENOISE_TX - 1)), ly = (int)(threadIdx.x / DENOISE_TX);
  const int i0 = (int)blockIdx.x * DENOISE_TX, row0 = (int)blockIdx.y * DENOISE_TY;
  const int i = i0 + lx, row = row0 + ly;
  const int w = (int)a.w, h = (int)a.h;  // sides <= 65536
  const int lw = DENOISE_TX + 2 * halo, lh = DENOISE_TY + 2 * halo;
  if (LDS) {
    float4* tx = denoise_tile;
    float4* tg = denoise_tile + lw * lh;
    for (int k = (int)threadIdx.x; k < lw * lh; k += DENOISE_BLOCK) {
      const int ty = k / lw, tcol = k - ty * lw;
      const int gy = row0 - halo + ty, gx = i0 - halo + tcol;
      if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
        const size_t q = (size_t)gy * a.w + (size_t)gx;
        tx[k] = a.X[q];
        tg[k] = a.G[q];
      }
    }
    __syncthreads();
  }
  if (i >= w || row >= h) return;
  const size_t p = (size_t)row * a.w + (size_t)i;
  const float4* tx = denoise_tile;
  const float4* tg = denoise_tile + lw * lh;
  const int lp = (ly + halo) * lw + (lx + halo);
  const float4 xp = LDS ? tx[lp] : a.X[p];
  const float4 gp = LDS ? tg[lp] : a.G[p];
  const float l_p = denoise_lum(xp);
  const float rz = 1.0f / (a.sz_step * fabsf(gp.w) + 1e-6f);
  const float rl = 1.0f / (a.sigma_l * sqrtf(xp.w) + 1e-4f);
  float sw = 0.0f, sx0 = 0.0f, sx1 = 0.0f, sx2 = 0.0f, sv = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = row + dy * step;
    if (qy < 0 || qy >= h) continue;
    const float hy = dy == 0 ? 0.375f : (dy == 1 || dy == -1 ? 0.25f : 0.0625f);
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = i + dx * step;
      if (qx < 0 || qx >= w) continue;
      const float hx = dx == 0 ? 0.375f : (dx == 1 || dx == -1 ? 0.25f : 0.0625f);
      float4 xq, gq;
      if (LDS) {
        const int lq = lp + dy * step * lw + dx * step;
        xq = tx[lq];
        gq = tg[lq];
      } else {
        const size_t q = (size_t)qy * a.w + (size_t)qx;
        xq = a.X[q];
        gq = a.G[q];
      }
      float wt = hx * hy;
      if (a.use_n) {
        const float e0 = gp.x - gq.x, e1 = gp.y - gq.y, e2 = gp.z - gq.z;
        const float dn2 = (e0 * e0 + e1 * e1) + e2 * e2;
        wt = wt * max0(1.0f - dn2 * a.k_n);
      }
      if (a.use_z) wt = wt * max0(1.0f - fabsf(gp.w - gq.w) * rz);
      const float l_q = denoise_lum(xq);
      if (a.use_l) wt = wt * max0(1.0f - fabsf(l_p - l_q) * rl);
      if (wt > 0.0f && l_q == l_q) {
        sw = sw + wt;
        sx0 = sx0 + wt * xq.x;
        sx1 = sx1 + wt * xq.y;
        sx2 = sx2 + wt * xq.z;
        sv = sv + (wt * wt) * xq.w;
      }
    }
  }
  float4 r = xp;
  if (sw > 0.0f) r = make_float4(sx0 / sw, sx1 / sw, sx2 / sw, sv / (sw * sw));
  if (FIN) {
    const float4 d = a.D[p];
    float* o = a.out + p * 3u;
    const bool live = d.w != 0.0f;
    o[0] = live ? r.x * d.x : 0.0f;
    o[1] = live ? r.y * d.y : 0.0f;
    o[2] = live ? r.z * d.z : 0.0f;
  } else {
    a.Y[p] = r;
  }
}

}  // namespace dev
}  // namespace rtw
