// rtw_ao_kernel.hpp — the ambient-occlusion / sky-visibility buffer (rtw_render_ao*): per pixel the sums over its camera
// rays of (open, cast) -- the AO rays of the first hit that reached `radius` unoccluded, and the AO rays cast.  One
// fused kernel in place of the chain rtw_camera_rays -> rtw_hit_rays -> a caller's hemisphere-ray kernel ->
// rtw_occluded_rays and a per-pixel sum: no ray, hit record, bound or answer goes through memory.  ao_kernel<KernelCfg K>
// is instantiated beside feature_kernel<K> and occluded_kernel<K> (make_variant, rtw_variants.hpp), so a scene's AO
// pass runs the walk its renders run, closest-hit for the camera ray and any-hit (trace_run<.., ANY>) for the AO rays.
//
// Per sample s of pixel (j, i): the ray and its stream word g_0 are camera_ray's (feature_kernel's), the record
// hit_kernel's for that ray (only p and the facing normal of it: hit_record<K.feat>, no F_UV, no material load).  A
// miss casts nothing and draws nothing.  A hit casts ao_rays rays, k = 0 .. ao_rays - 1 in order: the direction d_k and
// the next word g_{k+1} are scatter_kernel's for a Lambertian at that record with the stream word g_k (the generator
// seeded by xoro_seed(g_k); rs = rand_in_unit_sphere, d = n + unit(rs), near_zero(d) -> n: material.rs:42-56), whatever
// the real material is.  The AO ray is (p, d_k, the camera ray's time, stream g_{k+1}), its bound T = radius / |d_k| with
// |d_k| = sqrt((dx dx + dy dy) + dz dz), IEEE sqrt (sqrt_rn: its fast path falls back outside its proven range) and an
// IEEE division (plain `/`: once per AO ray, beside a tree walk), so radius = +inf or |d_k| = 0 give T = +inf.  Its
// answer is occluded_kernel's for that ray and T, with that kernel's set-up: no walk for T < TMIN or a best the
// always-tested list / trace_far already decided.  The sample adds (ao_rays - occluded, ao_rays), a miss (+0, +0).
//
// Mapping: feature_kernel's -- one wave per 8x8 tile, lane = pixel, a wave-uniform grid-stride loop over the tile
// slots, the node table filled once per workgroup, no barrier after the first.  Lanes that missed sit the AO walks
// out: the K loop is wave-uniform (ao_rays is a kernel argument), the `do .. while` around trace_run leaves for all
// active lanes together (quota = every active lane), as in occluded_kernel.
//
// One TraceState for both walks: the camera ray's walk has ended (its Best copied out, hit_record taken) before the
// first AO walk begins, and each AO walk ends before the next begins, so the stack column in LDS and the state's
// registers are reused; a second state would only add live registers to kernels that already spill around
// hit_record.  What lives across the K loop: p, n, the time, the generator word, the occluded count and k.
// The two sums stay in MEMORY between samples (feature_kernel's header: held in registers they doubled the scratch).
// Per-variant registers and scratch: DESIGN.md §4 "Ambient occlusion".
//
// The traversal guard is hit_kernel's: a trip in either walk ends the wave.  What it counts, wave-uniform, one atomic
// per counter word per wave at its end: counters[0] += the camera samples traced, counters[1] += the AO rays cast.
#pragma once
#include "../../include/rtw.h"
#include "rtw_query_kernel.hpp"

namespace rtw {

struct AoArgs {
  DevScene scene;
  DevCamera cam;
  float fw1, fh1, rw1, rh1, time_span;  // RenderArgs' (frame_args)
  uint32_t w, h, tiles_x, n_tiles;      // the frame, and its tile count
  uint64_t seed_hash;                   // splitmix64(seed)
  uint32_t sample_first, n_samples;
  uint32_t ao_rays;          // 1 .. 256 AO rays per hit
  float radius;              // > 0, +inf allowed
  const uint32_t* tile_ids;  // device array, or nullptr: slot k is tile k
  uint32_t n_slots;
  uint32_t packed;           // buffer [slot][64][2]; else the full w x h x 2 image
  float* ao;                 // 2 floats per pixel: (open, cast)
  uint32_t leaf16;           // RenderArgs::leaf16
  uint32_t spill_lanes;      // RenderArgs::spill_lanes
  int32_t* spill;            // RenderArgs::spill
  uint32_t* err;             // RenderArgs::err
  unsigned long long* counters;  // [0] += the camera samples traced, [1] += the AO rays cast
};

namespace dev {

template <KernelCfg K>
__global__ __launch_bounds__(K.blk) __attribute__((amdgpu_waves_per_eu(K.occ, 8))) void ao_kernel(AoArgs a) {
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
  unsigned long long traced = 0, cast = 0;  // wave-uniform
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
        uint64_t rng = camera_ray(a.cam, a.fw1, a.fh1, a.rw1, a.rh1, a.time_span, a.seed_hash, j, i, s, ray);
        TraceState ts;
        trace_begin<false, K.feat, K.stack, K.blk, K.codes16_stack(), K.far_lds_nodes()>(S, ray, ts, cnt, rng, stk16, stk,
                                                                                         a.err, nodes_lds);
        if constexpr (!(K.feat & F_LIST)) {
          // quota = every active lane, as hit_kernel: trace_run returns when all of them are done (or its guard tripped)
          do {
            const uint32_t act = (uint32_t)__popcll(__ballot(1));
            const uint32_t leaf_thr = (act * a.leaf16 + 15u) >> 4;
            trace_run<false, K.stack, K.spill, K.feat, K.blk, K.ncap, K.half, K.s16>(
                S, ray, ts, stk, spill, a.spill_lanes, cnt, act, leaf_thr, rng, a.err, ph + 4, nodes_lds, stk16);
          } while (ts.node >= 0 || ts.sp > 0);
          __builtin_amdgcn_s_setprio(0);  // trace_run raised it
        }
        const Best b = ts.b;
        tripped = b.prim == -2;  // trace_run / trace_far wrote the sticky error word
        const bool hit = b.prim >= 0;
        cast += (unsigned long long)__popcll(__ballot(hit)) * a.ao_rays;
        float f_open = 0.0f, f_cast = 0.0f;
        if (hit) {  // lanes that missed sit the AO walks out
          const Rec h = hit_record<K.feat>(S, ray, b, 0u);
          Ray ar;
          ar.o = h.p;
          ar.time = ray.time;
          const V3 n = h.n;
          uint32_t occluded = 0;
          for (uint32_t k = 0; k < a.ao_rays; ++k) {  // wave-uniform
            // scatter_kernel's Lambertian: the generator from the word, the rejection draw, unit(), material.rs:42-56
            rng = xoro_seed(rng);
            const V3 rs = rand_in_unit_sphere<false>(rng);
            V3 d = add(n, unit(rs));
            if (near_zero(d)) d = n;
            ar.d = d;
            const float T = a.radius / sqrt_rn(len2(d));  // IEEE sqrt and division: +inf for |d| = 0 or radius = +inf
            // occluded_kernel's walk for (ar, T), stream word g_{k+1}
            trace_begin<false, K.feat, K.stack, K.blk, K.codes16_stack(), K.far_lds_nodes()>(S, ar, ts, cnt, rng, stk16,
                                                                                             stk, a.err, nodes_lds);
            if constexpr (!(K.feat & F_LIST)) {
              // no walk for a bound below every BVH-mode candidate, nor once the always-tested list or trace_far answered
              const bool done = T < TMIN || (ts.b.prim >= 0 && !(ts.b.t > T));
              ts.node = done ? -1 : ts.node;
              do {
                const uint32_t act = (uint32_t)__popcll(__ballot(1));
                const uint32_t leaf_thr = (act * a.leaf16 + 15u) >> 4;
                trace_run<false, K.stack, K.spill, K.feat, K.blk, K.ncap, K.half, K.s16, true>(
                    S, ar, ts, stk, spill, a.spill_lanes, cnt, act, leaf_thr, rng, a.err, ph + 4, nodes_lds, stk16, T);
              } while (ts.node >= 0 || ts.sp > 0);
              __builtin_amdgcn_s_setprio(0);  // trace_run raised it
            }  // (list mode: trace_begin tested every primitive)
            tripped = tripped || ts.b.prim == -2;
            // the compare on the unseeded best: inclusive, and a NaN t (list mode's in-plane hit) passes it
            occluded += (ts.b.prim >= 0 && !(ts.b.t > T)) ? 1u : 0u;
            if (__any(tripped)) break;  // (the frame is invalid: the call reports RTW_EINVAL)
          }
          f_open = (float)(a.ao_rays - occluded);
          f_cast = (float)a.ao_rays;
        }
        // the sums stay in memory between samples (header comment): a lane re-reads what it alone wrote
        float* const p = a.ao + px * 2u;
        const float x = p[0], y = p[1];
        p[0] = x + f_open; p[1] = y + f_cast;
        if (__any(tripped)) break;
      }
    }
    // a corrupt tree: the wave stops after its first trip, as hit_kernel's
    if (__any(tripped)) break;
  }
  if (l == 0u) {
    if (traced) atomicAdd(a.counters, traced);
    if (cast) atomicAdd(a.counters + 1, cast);
  }
}

}  // namespace dev
}  // namespace rtw
