// rtw_feature_kernel.hpp — feature buffers for denoisers (rtw_render_features*): per pixel the sums over its camera
// rays of the first hit's albedo (3 f32), normal (3 f32) and depth (t, 1 | 0, 0: the second channel is the pixel's hit
// count).  One fused kernel in place of the chain rtw_camera_rays -> rtw_hit_rays -> rtw_scatter_rays and a per-pixel
// sum: no ray, hit or scatter record goes through memory.  feature_kernel<KernelCfg K> is instantiated beside
// hit_kernel<K> (make_variant, rtw_variants.hpp), so a scene's feature pass runs the walk its renders run.
//
// Per sample s of pixel (j, i): the ray is camera_ray's (rtw_query_kernel.hpp: rtw_camera_rays' ray for (seed, j, i, s),
// the stream word the generator's state after the time draw), the record hit_kernel's for that ray (trace_begin /
// trace_run with quota = every active lane, hit_record<K.feat | F_UV>), the albedo mat_attenuation<F_ALL> of the
// record's material (scatter_kernel's call: a Metal's colour whether or not the ray would be absorbed, a light's
// texture, (1,1,1) for a Dielectric), the background for a miss.  No draw beyond the camera's.  Each buffer holds
// x = x + f_s for s in sample order, one rounding per sample, added onto what it held.
//
// Mapping: one wave per 8x8 tile, lane l = pixel (l & 7, l >> 3) as tile_noise_kernel's; the loop over the tile slots is
// wave-uniform and grid-stride, the grid at most the resident capacity, the node table filled once per workgroup.  No
// barrier after the first: the waves of a workgroup finish at different times.  A lane off the image sits the tile
// out, a tile id beyond the frame is skipped; the 64 lanes trace 64 neighbouring pixels together, sample after sample.
//
// Registers: the eight sums stay in MEMORY between samples -- each sample ends with a read-modify-write of the pixel's
// eight floats, which a lane alone touches and which stays in L2 for the tile's few samples -- and the kernel keeps the
// variant's own waves per SIMD (K.occ), as hit_kernel does.  Held in registers across the sample loop, beside the
// walk's state, the sums, their three addresses and the loop's counters cost every default variant about twice the
// scratch (bytes per lane, sums in registers -> in memory: the 1024-lane sphere kernel 116 -> 64, the rect list kernel
// 108 -> 40, the 7-wave half-node mesh walk 144 -> 96; hit_kernel itself has 24, 0 and 36, sample_kernel 64, 0 and
// 56).  What is left is the walk's state spilled around hit_record<F_UV> and mat_attenuation<F_ALL>, outside the
// node loop.  The camera and frame constants are kernel arguments, re-read from SGPRs where the allocator wants them.
// The per-variant figures are in DESIGN.md §4 "Feature buffers".
//
// The traversal guard is hit_kernel's: the walk writes the sticky error word, and the wave stops after its first trip.
// What it counts: the samples it traced, one atomic per wave at its end onto the counters' first word.  No path queue,
// no sample buffer, no COUNT build.
#pragma once
#include "../../include/rtw.h"
#include "rtw_query_kernel.hpp"

namespace rtw {

struct FeatureArgs {
  DevScene scene;
  const DevShade* mshade;  // one shading record per material (Flat::mshade)
  DevCamera cam;
  float bg[3];
  float fw1, fh1, rw1, rh1, time_span;  // RenderArgs' (frame_args)
  uint32_t w, h, tiles_x, n_tiles;      // the frame, and its tile count
  uint64_t seed_hash;                   // splitmix64(seed)
  uint32_t sample_first, n_samples;
  const uint32_t* tile_ids;  // device array, or nullptr: slot k is tile k
  uint32_t n_slots;
  uint32_t packed;           // buffers [slot][64][c]; else the full w x h x c images
  float* albedo;             // 3 floats per pixel, or nullptr
  float* normal;             // 3 floats per pixel, or nullptr
  float* depth;              // 2 floats per pixel, or nullptr
  uint32_t leaf16;           // RenderArgs::leaf16
  uint32_t spill_lanes;      // RenderArgs::spill_lanes
  int32_t* spill;            // RenderArgs::spill
  uint32_t* err;             // RenderArgs::err
  unsigned long long* counters;  // [0] += the samples traced
};

namespace dev {

template <KernelCfg K>
__global__ __launch_bounds__(K.blk) __attribute__((amdgpu_waves_per_eu(K.occ, 8))) void feature_kernel(FeatureArgs a) {
  // hit_kernel's LDS: the stack columns and the node table
  __shared__ int32_t stk_all[K.stk_words()];
  __shared__ uint16_t stk16_all[K.stk16_words()];
  __shared__ float4 nodes_lds[K.lds_node_quads()];
  fill_nodes_lds<K>(a.scene, nodes_lds);
  __syncthreads();
  uint16_t* stk16 = stk16_all + threadIdx.x;
  int32_t* stk = stk_all + threadIdx.x;
  int32_t* spill = a.spill + (size_t)blockIdx.x * K.blk + threadIdx.x;  // unused unless the variant spills
  const DevScene& S = a.scene;
  uint32_t cnt[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // (COUNT builds only: never touched here)
  uint64_t ph[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  constexpr uint32_t WAVES = K.blk / 64;
  const uint32_t l = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t stride = gridDim.x * WAVES;
  unsigned long long traced = 0;  // wave-uniform
  for (uint32_t slot = blockIdx.x * WAVES + wave; slot < a.n_slots; slot += stride) {
    const uint32_t tile = a.tile_ids ? uload(a.tile_ids + slot) : slot;
    if (tile >= a.n_tiles) continue;  // wave-uniform
    const uint32_t ty = tile / a.tiles_x;
    const uint32_t i = (tile - ty * a.tiles_x) * 8u + (l & 7u), row = ty * 8u + (l >> 3);
    const bool in = i < a.w && row < a.h;
    bool tripped = false;
    traced += (unsigned long long)__popcll(__ballot(in)) * a.n_samples;
    if (in) {
      const uint32_t j = a.h - 1u - row;
      const size_t px = a.packed ? (size_t)slot * 64u + l : (size_t)row * a.w + i;
      const uint32_t s_end = a.sample_first + a.n_samples;
      for (uint32_t s = a.sample_first; s < s_end; ++s) {
        Ray ray;
        const uint64_t seg = camera_ray(a.cam, a.fw1, a.fh1, a.rw1, a.rh1, a.time_span, a.seed_hash, j, i, s, ray);
        TraceState ts;
        trace_begin<false, K.feat, K.stack, K.blk, K.codes16_stack(), K.far_lds_nodes()>(S, ray, ts, cnt, seg, stk16, stk,
                                                                                         a.err, nodes_lds);
        if constexpr (!(K.feat & F_LIST)) {
          // quota = every active lane, as hit_kernel: trace_run returns when all of them are done (or its guard tripped)
          do {
            const uint32_t act = (uint32_t)__popcll(__ballot(1));
            const uint32_t leaf_thr = (act * a.leaf16 + 15u) >> 4;
            trace_run<false, K.stack, K.spill, K.feat, K.blk, K.ncap, K.half, K.s16>(
                S, ray, ts, stk, spill, a.spill_lanes, cnt, act, leaf_thr, seg, a.err, ph + 4, nodes_lds, stk16);
          } while (ts.node >= 0 || ts.sp > 0);
          __builtin_amdgcn_s_setprio(0);  // trace_run raised it
        }
        const Best b = ts.b;
        tripped = b.prim == -2;  // trace_run / trace_far wrote the sticky error word
        V3 fa = ld3(a.bg), fn = mk(0.f, 0.f, 0.f);
        float fd = 0.f, fc = 0.f;
        if (b.prim >= 0) {
          const Rec h = hit_record<K.feat | F_UV>(S, ray, b, 1u << 12);
          const DevShade sh = a.mshade[h.mat];
          fa = mat_attenuation<F_ALL>(S, sh, mat_kind<F_ALL>(sh.kind), h, [&] { return ld3(sh.b); });
          fn = h.n;
          fd = b.t;
          fc = 1.0f;
        }
        // the sums stay in memory between samples (header comment): a lane re-reads what it alone wrote
        if (a.albedo) {
          float* const p = a.albedo + px * 3u;
          const float x = p[0], y = p[1], z = p[2];
          p[0] = x + fa.x; p[1] = y + fa.y; p[2] = z + fa.z;
        }
        if (a.normal) {
          float* const p = a.normal + px * 3u;
          const float x = p[0], y = p[1], z = p[2];
          p[0] = x + fn.x; p[1] = y + fn.y; p[2] = z + fn.z;
        }
        if (a.depth) {
          float* const p = a.depth + px * 2u;
          const float x = p[0], y = p[1];
          p[0] = x + fd; p[1] = y + fc;
        }
        if (__any(tripped)) break;  // (the frame is invalid: the call reports RTW_EINVAL)
      }
    }
    // a corrupt tree: the wave stops after its first trip, as hit_kernel's
    if (__any(tripped)) break;
  }
  if (l == 0u && traced) atomicAdd(a.counters, traced);
}

}  // namespace dev
}  // namespace rtw
