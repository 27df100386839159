// rtw_film_kernel.hpp — the film of a progressive render (rtw_render_samples_device, rtw_render_progressive,
// rtw_tonemap_device): accumulate_kernel is reduce_kernel (rtw_kernel.hip) continuing the sums a frame already holds,
// with the per-channel sum of squares beside them; tonemap_kernel is rtw_tonemap (console_app/src/main.rs:68-90) from a
// device sum image to a device RGB8 image.  Both stream: one thread per pixel, plain vector loads and stores, no LDS,
// no atomics.  The path kernels know nothing of either: a block of samples [B, B + 2^k) with B a multiple of 2^k is an
// ordinary pass of spp = 2^k whose key has B folded in on the host (frame_args; DESIGN.md §Progressive renders), and
// what these kernels need beyond RenderArgs they take as arguments of their own.  Included by rtw_kernel.hip alone.
#pragma once
#include "rtw_dev_math.hpp"

namespace rtw {
namespace dev {

constexpr int FILM_BLOCK = 256;

// x <- x + sample, in sample order, from the values already at a.out (lib.rs:83-87 continued); reduce_kernel's
// indexing: slot-major tiles (id table or first + k * stride), packed or full layout, lanes off the image and tiles
// beyond the frame return before they touch anything.  With sq_on, sq is a second image of a.out's layout and receives
// m <- m + (x * x) per channel in the same order: two roundings (the build's -ffp-contract=off).
__global__ __launch_bounds__(FILM_BLOCK) void accumulate_kernel(RenderArgs a, uint32_t n_slots, float* sq,
                                                                 uint32_t sq_on) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_slots * 64u) return;
  const uint32_t slot = g >> 6, l = g & 63u, gslot = a.slot_base + slot;
  const uint32_t tile = a.tile_ids ? a.tile_ids[gslot] : a.tile_first + gslot * a.tile_stride;
  const uint32_t i = (tile % a.tiles_x) * 8u + (l & 7u), row = (tile / a.tiles_x) * 8u + (l >> 3);
  if (i >= a.w || row >= a.h) return;
  const size_t at = a.packed_out ? ((size_t)gslot * 64u + l) * 3u : ((size_t)row * a.w + i) * 3u;
  float* o = a.out + at;
  float x = o[0], y = o[1], z = o[2];
  const float* q = a.sbuf + ((size_t)slot * a.spp * 64u + l) * 3u;
  if (sq_on) {
    float* m = sq + at;
    float mx = m[0], my = m[1], mz = m[2];
    for (uint32_t s = 0; s < a.spp; ++s, q += 64u * 3u) {
#if RTW_NT_SAMPLES
      const float sx = __builtin_nontemporal_load(q), sy = __builtin_nontemporal_load(q + 1),
                  sz = __builtin_nontemporal_load(q + 2);
#else
      const float sx = q[0], sy = q[1], sz = q[2];
#endif
      x = x + sx;
      y = y + sy;
      z = z + sz;
      mx = mx + sx * sx;
      my = my + sy * sy;
      mz = mz + sz * sz;
    }
    m[0] = mx;
    m[1] = my;
    m[2] = mz;
  } else {
    for (uint32_t s = 0; s < a.spp; ++s, q += 64u * 3u) {
#if RTW_NT_SAMPLES
      x = x + __builtin_nontemporal_load(q);
      y = y + __builtin_nontemporal_load(q + 1);
      z = z + __builtin_nontemporal_load(q + 2);
#else
      x = x + q[0];
      y = y + q[1];
      z = z + q[2];
#endif
    }
  }
  o[0] = x;
  o[1] = y;
  o[2] = z;
}

// rtw_tonemap's operations per channel: sqrt(scale * sum) with the host's scale = 1 / spp, f32::clamp(0, 0.999) (which
// keeps a NaN), then `as u8` of 255.999 c (saturating, NaN -> 0).  The IEEE sqrt is the build's default.
__device__ __forceinline__ uint8_t tonemap_channel(float sum, float scale) {
  const float c = sqrtf(scale * sum);
  const float cl = c < 0.0f ? 0.0f : (c > 0.999f ? 0.999f : c);
  const float x = 255.999f * cl;
  return (x != x || x <= 0.0f) ? (uint8_t)0 : (x >= 255.0f ? (uint8_t)255 : (uint8_t)x);
}

__global__ __launch_bounds__(FILM_BLOCK) void tonemap_kernel(const float* sum, uint32_t n_pixels, float scale,
                                                              uint8_t* rgb8) {
  const uint64_t g = (uint64_t)blockIdx.x * FILM_BLOCK + threadIdx.x;
  if (g >= n_pixels) return;
  const float* p = sum + g * 3u;
  uint8_t* o = rgb8 + g * 3u;
  const float r = p[0], gr = p[1], b = p[2];
  o[0] = tonemap_channel(r, scale);
  o[1] = tonemap_channel(gr, scale);
  o[2] = tonemap_channel(b, scale);
}

}  // namespace dev
}  // namespace rtw
