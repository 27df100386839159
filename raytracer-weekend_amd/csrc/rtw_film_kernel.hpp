// rtw_film_kernel.hpp — the film of a progressive render (rtw_render_samples_device, rtw_render_progressive,
// rtw_tonemap_device): accumulate_kernel is reduce_kernel (rtw_kernel.hip) continuing the sums a frame already holds,
// with the per-channel sum of squares beside them; tonemap_kernel is rtw_tonemap (console_app/src/main.rs:68-90) from a
// device sum image to a device RGB8 image.  Both stream: one thread per pixel, plain vector loads and stores, no LDS,
// no atomics.  Behind them the adaptive render's kernels (rtw_tile_noise_device, rtw_render_adaptive*): tile_noise_kernel
// turns the two sums into a per-tile error, compact_tiles_kernel keeps the ids of the tiles above the threshold, and
// tonemap_tiles_kernel is the tonemap with a sample count per tile.
// The path kernels know nothing of any of them: a block of samples [B, B + 2^k) with B a multiple of 2^k is an
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

// ---- adaptive sampling (rtw_tile_noise_device, rtw_render_adaptive*, rtw_tonemap_tiles_device)

// The f32 sum of a wave's 64 values by the fixed butterfly: at level k = 0..5 x[i] = x[i] + x[i ^ (1 << k)], i.e. the
// adjacent-pair tree.  The order is the contract (the tests restate it); every lane of the wave must be here, and all
// end with the same value.
__device__ __forceinline__ float wave_tree_sum(float x) {
#pragma unroll
  for (int k = 0; k < 6; ++k) x = x + __shfl_xor(x, 1 << k, 64);
  return x;
}

// One wave per tested tile (slot k of ids_in, or tile k without a table), lane l = pixel (l & 7, l >> 3) of the tile,
// accumulate_kernel's indexing over the full w x h x 3 layout.  From the sums and sums of squares of `samples` = n
// samples per pixel, inv = 1 / n the host's: per in-image lane and channel m = s inv, v = q inv - m m clamped at 0 (a
// NaN stays), e = (v0 + v1) + v2, l = (m0 + m1) + m2; lanes off the image give e = l = +0.  With E, L the wave's tree
// sums and Pf the tile's in-image pixels: err = sqrt((E inv) / Pf) / (|L| / Pf + 0.03).  All f32, one rounding per
// operation (-ffp-contract=off), IEEE sqrt and division.  The tile is converged iff err <= threshold (never for a NaN).
// Lane 0 writes err[tile] (err may be NULL), tile_samples[tile] = n (may be NULL) and the slot's flag, 1 = not
// converged, which compact_tiles_kernel turns into the list.  A slot whose id is beyond the last tile gets flag 0 and
// nothing else.  No LDS, no atomics.
__global__ __launch_bounds__(FILM_BLOCK) void tile_noise_kernel(const float* sum, const float* sq, uint32_t w,
                                                                 uint32_t h, uint32_t tiles_x, uint32_t n_tiles,
                                                                 const uint32_t* ids_in, uint32_t n_in,
                                                                 uint32_t samples, float inv, float threshold,
                                                                 float* err, uint32_t* tile_samples,
                                                                 uint32_t* flags) {
  const uint64_t slot = (uint64_t)blockIdx.x * (FILM_BLOCK / 64u) + (threadIdx.x >> 6);
  const uint32_t l = threadIdx.x & 63u;
  if (slot >= n_in) return;  // (wave-uniform)
  const uint32_t tile = ids_in ? ids_in[slot] : (uint32_t)slot;
  if (tile >= n_tiles) {
    if (l == 0u) flags[slot] = 0u;
    return;
  }
  const uint32_t i0 = (tile % tiles_x) * 8u, row0 = (tile / tiles_x) * 8u;
  const uint32_t i = i0 + (l & 7u), row = row0 + (l >> 3);
  float e = 0.0f, lum = 0.0f;
  if (i < w && row < h) {
    const size_t at = ((size_t)row * w + i) * 3u;
    const float* s = sum + at;
    const float* q = sq + at;
    const float m0 = s[0] * inv, m1 = s[1] * inv, m2 = s[2] * inv;
    float v0 = q[0] * inv - m0 * m0, v1 = q[1] * inv - m1 * m1, v2 = q[2] * inv - m2 * m2;
    v0 = v0 < 0.0f ? 0.0f : v0;
    v1 = v1 < 0.0f ? 0.0f : v1;
    v2 = v2 < 0.0f ? 0.0f : v2;
    e = (v0 + v1) + v2;
    lum = (m0 + m1) + m2;
  }
  const float E = wave_tree_sum(e), L = wave_tree_sum(lum);
  const uint32_t pw = w - i0 < 8u ? w - i0 : 8u, ph = h - row0 < 8u ? h - row0 : 8u;
  const float Pf = (float)(pw * ph);
  const float num = sqrtf((E * inv) / Pf);
  const float den = fabsf(L) / Pf + 0.03f;
  const float r = num / den;
  if (l == 0u) {
    if (err) err[tile] = r;
    if (tile_samples) tile_samples[tile] = samples;
    flags[slot] = r <= threshold ? 0u : 1u;
  }
}

// The stable compaction behind tile_noise_kernel: the ids (ids_in[k], or k without a table) of the slots whose flag
// is set, in slot order, to the front of `io`, which holds the flags on entry, and their number to *n_out.  One
// workgroup, in place: a round takes COMPACT_BLOCK * 32 slots, thread t the 32 consecutive ones from base + 32 t, as a
// mask in a register.  Every write of a round goes to a position at or before its slot, hence before the next round's
// flags, and after the barrier behind the round's own reads.  The block scan of the 1024 counts is Hillis-Steele in
// LDS.  ids_in must not overlap io.
constexpr int COMPACT_BLOCK = 1024;
__global__ __launch_bounds__(COMPACT_BLOCK) void compact_tiles_kernel(const uint32_t* ids_in, uint32_t n_in,
                                                                       uint32_t* io, uint32_t* n_out) {
  __shared__ uint32_t scan[COMPACT_BLOCK];
  const uint32_t t = threadIdx.x;
  uint32_t total = 0;
  for (uint64_t base = 0; base < n_in; base += (uint64_t)COMPACT_BLOCK * 32u) {
    const uint64_t first = base + (uint64_t)t * 32u;
    uint32_t mask = 0;
    for (uint32_t j = 0; j < 32u; ++j)
      if (first + j < n_in && io[first + j]) mask |= 1u << j;
    const uint32_t mine = (uint32_t)__builtin_popcount(mask);
    scan[t] = mine;
    __syncthreads();  // (also: every flag of the round has been read)
    for (uint32_t d = 1; d < (uint32_t)COMPACT_BLOCK; d <<= 1) {
      const uint32_t add = t >= d ? scan[t - d] : 0u;
      __syncthreads();
      scan[t] += add;
      __syncthreads();
    }
    uint32_t pos = total + scan[t] - mine;
    for (uint32_t j = 0; j < 32u; ++j)
      if (mask >> j & 1u) io[pos++] = ids_in ? ids_in[first + j] : (uint32_t)(first + j);
    total += scan[COMPACT_BLOCK - 1];
    __syncthreads();  // scan[] is rewritten by the next round
  }
  if (t == 0u) *n_out = total;
}

// rtw_tonemap per 8x8 tile: the pixels of tile t with scale = 1 / tile_samples[t] (the host's operation; IEEE division
// here as there), black for a tile without samples.  One thread per pixel of the full w x h image.
__global__ __launch_bounds__(FILM_BLOCK) void tonemap_tiles_kernel(const float* sum, uint32_t w, uint32_t h,
                                                                    uint32_t tiles_x, const uint32_t* tile_samples,
                                                                    uint8_t* rgb8) {
  const uint64_t g = (uint64_t)blockIdx.x * FILM_BLOCK + threadIdx.x;
  if (g >= (uint64_t)w * h) return;
  const uint32_t row = (uint32_t)(g / w), i = (uint32_t)(g - (uint64_t)row * w);
  const uint32_t n = tile_samples[(row >> 3) * tiles_x + (i >> 3)];
  const float* p = sum + g * 3u;
  uint8_t* o = rgb8 + g * 3u;
  if (n == 0u) {
    o[0] = o[1] = o[2] = 0;
    return;
  }
  const float scale = 1.0f / (float)n;
  const float r = p[0], gr = p[1], b = p[2];
  o[0] = tonemap_channel(r, scale);
  o[1] = tonemap_channel(gr, scale);
  o[2] = tonemap_channel(b, scale);
}

}  // namespace dev
}  // namespace rtw
