// rtw_variants.hpp — the path kernel's variants as the host names them: Variant (both entry points of a
// configuration, its ray-query, occlusion-query, radiance-query, feature-buffer and ambient-occlusion kernels, and the KernelCfg the launch is sized from), make_variant, the tuning Knobs, the named configurations,
// and pick5, the 5-wave selection per feature set.  rtw_kernel.hip's pick_kernel instantiates every variant but the
// F_MESHES ones, which rtw_kernel_mesh.hip's pick_mesh instantiates under its own compiler flags.
#pragma once
#include <stdio.h>

#include "rtw_path_kernel.hpp"
#include "rtw_query_kernel.hpp"
#include "rtw_occluded_kernel.hpp"
#include "rtw_sample_kernel.hpp"
#include "rtw_feature_kernel.hpp"
#include "rtw_ao_kernel.hpp"

namespace rtw {

typedef void (*path_fn)(RenderArgs);
typedef void (*hit_fn)(QueryArgs);
typedef void (*occluded_fn)(OccludedArgs);
typedef void (*sample_fn)(SampleArgs);
typedef void (*feature_fn)(FeatureArgs);
typedef void (*ao_fn)(AoArgs);
using dev::KernelCfg;
struct Variant {
  path_fn fn[2];  // the kernel and its COUNT build (fn[count])
  hit_fn hit;     // the ray-query kernel over the same walk (rtw_query_kernel.hpp; no COUNT build)
  occluded_fn occluded;  // the occlusion-query kernel: any hit to the caller's t_max (rtw_occluded_kernel.hpp)
  sample_fn sample;  // the radiance-query kernel: whole paths for caller rays (rtw_sample_kernel.hpp; no COUNT build)
  feature_fn feature;  // the feature-buffer kernel: first-hit albedo, normal, depth per pixel (rtw_feature_kernel.hpp)
  ao_fn ao;  // the ambient-occlusion kernel: a closest-hit walk, then any-hit walks from the hit (rtw_ao_kernel.hpp)
  KernelCfg cfg;  // what they were compiled for: the launch (grid, stack / spill split, batch) is sized from it
};
template <KernelCfg K>  // the only way a Variant is made
static Variant make_variant() {
  return {{dev::path_kernel<false, K>, dev::path_kernel<true, K>}, dev::hit_kernel<K>, dev::occluded_kernel<K>,
          dev::sample_kernel<K>, dev::feature_kernel<K>, dev::ao_kernel<K>, K};
}
constexpr KernelCfg with_half(KernelCfg k) { k.half = true; return k; }    // ... reading the half-precision nodes
constexpr KernelCfg with_spill(KernelCfg k) { k.spill = true; return k; }  // ... with the HBM stack spill

// A tuning knob: unset, or its value.  Knobs holds every knob rtw_kernel.hip reads, filled once per
// render / introspection call by read_knobs(): the selection and the launch parameters take them from there.
struct Knob {
  bool set = false;
  int v = 0;
  int get(int dflt) const { return set ? v : dflt; }
};
struct Knobs {
  Knob stack_lds, half_nodes, generic, list_all, list_occ, occ, ldsn_waves, lds_nodes, ldsn_blk, mesh_s16;  // selection
  Knob batch, quota16, leaf16, regen_min, pass_log2;                                                        // launch
  Knob tile_lists, tile_list_cap;  // the per-tile lists of camera rays (0 = off; 1..15 candidates per tile)
  bool verbose = false;
};

// The configurations the selection below names.  The 32-bit-stack walks over global nodes, per feature set F:
template <uint32_t F> constexpr KernelCfg WALK4{.stack = dev::STACK_LDS, .spill = false, .occ = 4, .feat = F};
template <uint32_t F> constexpr KernelCfg WALK5{.stack = dev::STACK_LDS5, .spill = false, .occ = 5, .feat = F};
template <uint32_t F> constexpr KernelCfg DEEP5{.stack = dev::STACK_DEEP5, .spill = false, .occ = 5, .feat = F};
constexpr KernelCfg SPHERES6{.stack = dev::STACK_LDS5, .spill = false, .occ = 6, .feat = F_SPHERES};
// a 4-entry LDS stack, so that the HBM spill path runs on every scene (RTW_STACK_LDS=4)
constexpr KernelCfg SPILL_TEST{.stack = 4, .spill = true, .occ = 4, .feat = F_ALL};
// no BVH (list mode): variants without the walk
constexpr KernelCfg LIST_ALL{.stack = 1, .spill = false, .occ = 5, .feat = F_ALL | F_LIST};
constexpr KernelCfg LIST_BOXES8{.stack = 1, .spill = false, .occ = 8, .feat = F_BOXES | F_LIST};
constexpr KernelCfg LIST_BOXES6{.stack = 1, .spill = false, .occ = 6, .feat = F_BOXES | F_LIST};
// LDS-node variants: the node table lives in each workgroup's LDS.  512-lane workgroups at 6
// waves/SIMD = 3 per CU: 24 rows of 16-bit stack entries x 512 x 2 B + 224 node4s x 128 B + the pool
// words = 53,440 B per workgroup, 160,320 B per CU (<= 160 KiB): sphere worlds of up to ~850 spheres.
// (The spheres' 32-B test records in LDS too -- 18 stack rows, 512 x 32 B -- and the winner's hit record
// from them measured equal within 0.2%: profiles/r02/experiments n6, h2.)
constexpr KernelCfg LDSN_224{.stack = 24, .spill = false, .occ = 6, .feat = F_SPHERES, .blk = 512, .ncap = 224};
// 8 waves per SIMD when the tree fits a smaller table: 512-lane workgroups x 4 per CU, 144 node4s and 16
// stack rows in 36 KB of LDS, 64 VGPRs (the compiler spills 32 B per lane to scratch, outside the node
// loop).  The latency-bound kernel gains from the extra waves: jumpy-1080p 26.34k -> 27.02k Mrays/s
// (profiles/r03/experiments, w1); 7 waves (448-lane workgroups, 160 node4s, 18 rows, 72 VGPRs) measured
// slower (25.18k), as did both with half-precision nodes.  Knob RTW_LDSN_WAVES (6, 7, 8).
constexpr KernelCfg LDSN_512{.stack = 16, .spill = false, .occ = 8, .feat = F_SPHERES, .blk = 512, .ncap = 144};
constexpr KernelCfg LDSN_448{.stack = 18, .spill = false, .occ = 7, .feat = F_SPHERES, .blk = 448, .ncap = 160};
// 1024-lane workgroups x 2 per CU (knob RTW_LDSN_BLK, 512 = the 4 x 512 form): one node table per 16
// waves, and the LDS this frees holds the waves' start rings (path_kernel SRING, KernelCfg::ldsn_ring).  LDS per
// workgroup: 18 KB nodes + 32 KB stack + 28 KB rings.  (Until round 7 it held the paths' T / depth / id, 20 KB of
// state rows: fewer scratch spills, throughput unchanged; profiles/r07/experiments records that form.)
constexpr KernelCfg LDSN_1024{.stack = 16, .spill = false, .occ = 8, .feat = F_SPHERES, .blk = 1024, .ncap = 144};
// The mesh walk with 16-bit stack entries (the nodes' codes: half the LDS of the 32-bit stack, whose 31 KB per
// workgroup allow 5 per CU) and the paths' T / depth / id in LDS state rows, at 6 or 7 waves / SIMD (knob
// RTW_MESH_S16; 0 = the 32-bit stack at 5).  Measured (r04n, r04p): monument-4k +3.0% at 6 waves (80 VGPRs), +2.2%
// more with the state rows (scratch 40 -> 32 B), 7 waves slower; cow-1080p -4.1% / -0.7% with the rows.  With the
// start_path operands in LDS (round 5, m1) the SGPR overflow is gone and 7 waves (72 VGPRs) win: monument
// +2.3%, cow +0.8% over 6 (profiles/r05/experiments, m2), so every tree with half nodes takes the 7-wave walk.
template <uint32_t F>
constexpr KernelCfg S16_7{.stack = dev::STACK_DEEP5, .spill = false, .occ = 7, .feat = F, .s16 = true};
template <uint32_t F>
constexpr KernelCfg S16_6{.stack = dev::STACK_DEEP5, .spill = false, .occ = 6, .feat = F, .s16 = true};

template <uint32_t F>
static Variant pick5(const Knobs& kn, uint32_t need, bool half = false, bool codes16 = false) {
  using namespace dev;
  if constexpr (F == F_MESHES) {
    int s16 = kn.mesh_s16.get(half ? 7 : 0);
    if (s16 != 0 && s16 != 6 && s16 != 7) {  //  no silent fallback for a value no variant has
      fprintf(stderr, "rtw: RTW_MESH_S16=%d ignored (0, 6 or 7)\n", s16);
      s16 = half ? 7 : 0;
    }
    if (codes16 && s16 != 0 && need <= (uint32_t)STACK_DEEP5) {
      if (s16 == 7) return half ? make_variant<with_half(S16_7<F>)>() : make_variant<S16_7<F>>();
      return half ? make_variant<with_half(S16_6<F>)>() : make_variant<S16_6<F>>();
    }
  }
  if constexpr (F == F_MESHES) {  // the half-precision node table (DevNode4h) where it was built
    if (half && need <= (uint32_t)STACK_LDS5) return make_variant<with_half(WALK5<F>)>();
    if (half && need <= (uint32_t)STACK_DEEP5) return make_variant<with_half(DEEP5<F>)>();
  }
  if (need <= (uint32_t)STACK_LDS5) return make_variant<WALK5<F>>();
  if constexpr (F == F_MESHES || F == F_ALL) {
    if (need <= (uint32_t)STACK_DEEP5) return make_variant<DEEP5<F>>();
    return make_variant<with_spill(DEEP5<F>)>();
  }
  return make_variant<with_spill(WALK5<F>)>();
}
// The mesh variants (F_MESHES) are compiled in their own translation unit, rtw_kernel_mesh.hip, with the
// iterative-ILP machine scheduler instead of max-ILP (Makefile KFLAGS_MESH): cow +0.6%, monument +1.2%, where the
// sphere and list-mode kernels lose 0.7-0.8% with it (profiles/r04/experiments k1)
Variant pick_mesh(const Knobs& kn, uint32_t need, bool half, bool codes16);

}  // namespace rtw
