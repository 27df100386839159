// rtw_query_kernel.hpp — closest-hit ray queries: Hittable::hit on the world list (hittable/mod.rs:22-69) for rays
// the caller chooses, instead of the camera paths of path_kernel.  hit_kernel<KernelCfg K> is instantiated beside
// path_kernel<COUNT, K> (make_variant, rtw_variants.hpp), so a scene's queries run the walk and feature set its
// renders run: the list loops, the 32-bit, 16-bit (S16), half-node and LDS-node walks, the HBM stack spill, trace_far.
//
// A query is world.hit(ray, 0.001, +inf): lib.rs:102's interval, the only one the culling pads, the far bound and the
// list loops' NaN rule are proven for.  Caller-chosen t_min / t_max are not offered here (occluded_kernel,
// rtw_occluded_kernel.hpp, takes a t_max for its yes / no answer).  The winner is the render's: ties
// to the later object, BvhNode groups as sets, the in-plane (NaN) hit reported by the list-mode loops only
// (DESIGN.md §2).  rtw_ray::stream is the segment word that keys ConstantMedium's free-path sub-stream.
//
// What it shares with path_kernel: the LDS stack columns and node table of K, trace_begin, trace_run, hit_record.
// What it leaves out: the path queue, id pool and start ring, StartArgs, shading, the sample buffer, COUNT builds.
#pragma once
#include "../../include/rtw.h"
#include "rtw_path_kernel.hpp"

namespace rtw {

struct QueryArgs {
  DevScene scene;
  const void* rays;      // rtw_ray[n], 16-byte aligned
  void* hits;            // rtw_hit[n], 16-byte aligned
  uint64_t n;
  float time_lo, time_hi;  // the committed motion range (Flat): a ray outside it is not traced (RTW_HIT_BAD_RAY)
  uint32_t leaf16;       // RenderArgs::leaf16
  uint32_t spill_lanes;  // RenderArgs::spill_lanes
  int32_t* spill;        // RenderArgs::spill
  uint32_t* err;         // RenderArgs::err
};

namespace dev {

static_assert(sizeof(rtw_ray) == 40 && sizeof(rtw_hit) == 48, "rtw_ray / rtw_hit layout (include/rtw.h)");
// a ray record starts on an 8-byte boundary (40 B each): its two 16-byte quads and the stream word
typedef float ray_quad __attribute__((ext_vector_type(4), aligned(8)));
typedef uint32_t ray_pair __attribute__((ext_vector_type(2), aligned(8)));
// the record as it lies in memory (returned by value: with the quads as reference parameters sample_kernel's list and
// mesh variants came out as other code, one with scratch; scripts/isa_diff.sh)
struct RayRec {
  ray_quad q0, q1;  // origin, direction.x | direction.y, .z, time, reserved
  ray_pair q2;      // stream
};
__device__ __forceinline__ RayRec load_ray(const void* rays, uint64_t i) {
  const char* rp = reinterpret_cast<const char*>(rays) + i * sizeof(rtw_ray);
  RayRec r;
  r.q0 = *reinterpret_cast<const ray_quad*>(rp);
  r.q1 = *reinterpret_cast<const ray_quad*>(rp + 16);
  r.q2 = *reinterpret_cast<const ray_pair*>(rp + 32);
  return r;
}
__device__ __forceinline__ void store_ray(void* rays, uint64_t i, const RayRec& r) {
  char* rp = reinterpret_cast<char*>(rays) + i * sizeof(rtw_ray);
  *reinterpret_cast<ray_quad*>(rp) = r.q0;
  *reinterpret_cast<ray_quad*>(rp + 16) = r.q1;
  *reinterpret_cast<ray_pair*>(rp + 32) = r.q2;
}
// the record as the walk takes it: the Ray, and the stream word returned
__device__ __forceinline__ uint64_t ray_of(const RayRec& r, Ray& ray) {
  ray.o = mk(r.q0.x, r.q0.y, r.q0.z);
  ray.d = mk(r.q0.w, r.q1.x, r.q1.y);
  ray.time = r.q1.z;
  return ((uint64_t)r.q2.y << 32) | r.q2.x;
}
__device__ __forceinline__ uint64_t load_ray(const void* rays, uint64_t i, Ray& ray) {
  return ray_of(load_ray(rays, i), ray);
}

// start_path's ray (rtw_path_kernel.hpp, AB = false; lib.rs:84-86 + camera.rs:66-74) for pixel (j, i), sample s: the
// generator keyed by (seed_hash, j, i, s), its draws in start_path's order (u, v, the lens disk, the time) and the same
// f32 operations; fw1 .. time_span are RenderArgs'.  -> the generator's state after the time draw (the stream word).
// The one body camera_rays_kernel (rtw_shade_kernel.hpp) and feature_kernel (rtw_feature_kernel.hpp) both call.
__device__ __forceinline__ uint64_t camera_ray(const DevCamera& C, float fw1, float fh1, float rw1, float rh1,
                                               float time_span, uint64_t seed_hash, uint32_t j, uint32_t i, uint32_t s,
                                               Ray& ray) {
  uint64_t rng = xoro_seed(splitmix64(seed_hash ^ (((uint64_t)j << 48) | ((uint64_t)i << 32) | s)));
  const float u = div_by_recip((float)i + gen_f32(rng), fw1, rw1);
  const float v = div_by_recip((float)j + gen_f32(rng), fh1, rh1);
  const V3 rd = scale(rand_in_unit_disk<false>(rng), C.lens_radius);
  const V3 off = add(scale(ld3(C.u), rd.x), scale(ld3(C.v), rd.y));
  ray.o = add(ld3(C.origin), off);
  ray.d = sub(sub(add(add(ld3(C.llc), scale(ld3(C.horizontal), u)), scale(ld3(C.vertical), v)), ld3(C.origin)), off);
  ray.time = gen_range<false>(rng, C.time0, C.time1, time_span);
  return rng;
}

// Each lane owns one ray and a wave takes 64 consecutive ones (the caller's order decides coherence); grid-stride
// over n, the grid at most the resident capacity, so an LDS-node workgroup copies its node table once.  The last
// wave runs partial under its exec mask.
template <KernelCfg K>
__global__ __launch_bounds__(K.blk) __attribute__((amdgpu_waves_per_eu(K.occ, 8))) void hit_kernel(QueryArgs a) {
  // path_kernel's LDS without the LST rows: the stack columns (+ 1: trace_run's branch-free push) and the node table
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
      // the BVH's moving-sphere boxes bound [time_lo, time_hi] only: a NaN time fails both compares
      const bool bad = !(ray.time >= a.time_lo && ray.time <= a.time_hi);
      float4 o0 = make_float4(0.f, 0.f, 0.f, 0.f), o1 = make_float4(0.f, 0.f, INFINITY, 0.f);
      uint32_t mat = 0u, key = 0u, flags = bad ? (uint32_t)RTW_HIT_BAD_RAY : 0u;
      float v = 0.f;
      if (!bad) {
        TraceState ts;
        trace_begin<false, K.feat, K.stack, K.blk, K.codes16_stack(), K.far_lds_nodes()>(S, ray, ts, cnt, seg, stk16, stk,
                                                                                         a.err, nodes_lds);
        if constexpr (!(K.feat & F_LIST)) {
          // quota = every active lane: trace_run returns when all of them are done (or its guard tripped)
          do {
            const uint32_t act = (uint32_t)__popcll(__ballot(1));
            const uint32_t leaf_thr = (act * a.leaf16 + 15u) >> 4;
            trace_run<false, K.stack, K.spill, K.feat, K.blk, K.ncap, K.half, K.s16>(
                S, ray, ts, stk, spill, a.spill_lanes, cnt, act, leaf_thr, seg, a.err, ph + 4, nodes_lds, stk16);
          } while (ts.node >= 0 || ts.sp > 0);
          __builtin_amdgcn_s_setprio(0);  // trace_run raised it
        }  // (list mode: trace_begin tested every primitive)
        const Best b = ts.b;
        tripped = b.prim == -2;  // trace_run / trace_far wrote the sticky error word
        if (b.prim >= 0) {
          // the whole HitRecord, the sphere's uv included (spherical.rs:62-77 computes it for every hit)
          const Rec h = hit_record<K.feat | F_UV>(S, ray, b, 1u << 12);
          o0 = make_float4(h.p.x, h.p.y, h.p.z, h.n.x);
          o1 = make_float4(h.n.y, h.n.z, b.t, h.u);
          v = h.v;
          mat = h.mat;
          key = S.prims[b.prim].key;
          flags = (uint32_t)RTW_HIT_HIT | (h.front ? (uint32_t)RTW_HIT_FRONT_FACE : 0u);
        }
      }
      float4* hp = reinterpret_cast<float4*>(reinterpret_cast<char*>(a.hits) + i * sizeof(rtw_hit));
      hp[0] = o0;
      hp[1] = o1;
      hp[2] = make_float4(v, __uint_as_float(mat), __uint_as_float(key), __uint_as_float(flags));
    }
    // a corrupt tree (the call reports RTW_EINVAL and its records are invalid): the wave stops after its first trip,
    // 2^20 node-loop iterations, so the grid drains after one trip per wave
    if (__any(tripped)) break;
  }
}

}  // namespace dev
}  // namespace rtw
