// rtw_occluded_kernel.hpp — occlusion ray queries: world.hit(ray, 0.001, t_max).is_some() (hittable/mod.rs:57-69) for
// rays and bounds the caller chooses: shadow rays, ambient occlusion, visibility between two points.
// occluded_kernel<KernelCfg K> is instantiated beside hit_kernel<K> (make_variant, rtw_variants.hpp), so a scene's
// occlusion queries run the walk its renders and closest-hit queries run.
//
// The answer for ray k with bound T = t_max[k] (+inf without the array) is defined on the record hit_kernel returns
// for that ray: occluded = hit && !(t > T).  The bound is inclusive, as the reference's primitives reject with
// t > t_max; a NaN t (the in-plane rect hit of the list-mode loops) occludes for every T; T < 0.001 is free but for
// that case.  It is found without the record: Best stays unseeded (+inf), and T enters in two places only, both in
// trace_run<.., ANY> (rtw_dev_trace.hpp): a lane retires as soon as its best is within T, and the slab tests cull at
// min(best t, T).  A list-mode variant tests every primitive in trace_begin and is decided afterwards, as are the
// far-origin lanes (trace_far) and a lane whose always-tested list already answered.  T < 0.001 takes no BVH walk:
// every candidate a BVH-mode test accepts has t >= 0.001.
//
// What it shares with hit_kernel: the LDS (stack columns, node table), the grid-stride shape, launch bounds and the
// traversal guard.  What it leaves out: hit_record and the 48-byte record; it stores one byte per ray.
#pragma once
#include "rtw_query_kernel.hpp"

namespace rtw {

struct OccludedArgs {
  DevScene scene;
  const void* rays;      // rtw_ray[n], 16-byte aligned
  const float* t_max;    // float[n], or NULL: +inf for every ray
  uint8_t* occluded;     // uint8_t[n]
  uint64_t n;
  float time_lo, time_hi;  // the committed motion range (Flat): a ray outside it is not traced (RTW_OCCLUDED_BAD_RAY)
  uint32_t leaf16;       // RenderArgs::leaf16
  uint32_t spill_lanes;  // RenderArgs::spill_lanes
  int32_t* spill;        // RenderArgs::spill
  uint32_t* err;         // RenderArgs::err
};

namespace dev {

template <KernelCfg K>
__global__ __launch_bounds__(K.blk) __attribute__((amdgpu_waves_per_eu(K.occ, 8))) void occluded_kernel(OccludedArgs a) {
  // hit_kernel's LDS: the stack columns (+ 1: trace_run's branch-free push) and the node table
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
  const uint64_t stride = (uint64_t)gridDim.x * K.blk;
  // wave-uniform: the wave's first ray
  for (uint64_t base = (uint64_t)blockIdx.x * K.blk + (threadIdx.x & ~63u); base < a.n; base += stride) {
    const uint64_t i = base + (threadIdx.x & 63u);
    bool tripped = false;
    if (i < a.n) {
      Ray ray;
      const uint64_t seg = load_ray(a.rays, i, ray);
      const float T = a.t_max ? a.t_max[i] : INFINITY;
      // a NaN time fails both compares (hit_kernel); a NaN bound answers nothing
      const bool bad = !(ray.time >= a.time_lo && ray.time <= a.time_hi) || T != T;
      uint32_t out = bad ? (uint32_t)RTW_OCCLUDED_BAD_RAY : 0u;
      if (!bad) {
        TraceState ts;
        trace_begin<false, K.feat, K.stack, K.blk, K.codes16_stack(), K.far_lds_nodes()>(S, ray, ts, cnt, seg, stk16, stk,
                                                                                         a.err, nodes_lds);
        if constexpr (!(K.feat & F_LIST)) {
          // no walk for a bound below every BVH-mode candidate, nor once the always-tested list or trace_far answered
          const bool done = T < TMIN || (ts.b.prim >= 0 && !(ts.b.t > T));
          ts.node = done ? -1 : ts.node;
          // quota = every active lane: trace_run returns when all of them are done (or its guard tripped)
          do {
            const uint32_t act = (uint32_t)__popcll(__ballot(1));
            const uint32_t leaf_thr = (act * a.leaf16 + 15u) >> 4;
            trace_run<false, K.stack, K.spill, K.feat, K.blk, K.ncap, K.half, K.s16, true>(
                S, ray, ts, stk, spill, a.spill_lanes, cnt, act, leaf_thr, seg, a.err, ph + 4, nodes_lds, stk16, T);
          } while (ts.node >= 0 || ts.sp > 0);
          __builtin_amdgcn_s_setprio(0);  // trace_run raised it
        }  // (list mode: trace_begin tested every primitive)
        const Best b = ts.b;
        tripped = b.prim == -2;  // trace_run / trace_far wrote the sticky error word
        // the compare on the unseeded best: inclusive, and a NaN t (list mode's in-plane hit) passes it
        out = (b.prim >= 0 && !(b.t > T)) ? (uint32_t)RTW_OCCLUDED_HIT : 0u;
      }
      a.occluded[i] = (uint8_t)out;
    }
    // a corrupt tree (the call reports RTW_EINVAL and its answers are invalid): the wave stops after its first trip
    if (__any(tripped)) break;
  }
}

}  // namespace dev
}  // namespace rtw
