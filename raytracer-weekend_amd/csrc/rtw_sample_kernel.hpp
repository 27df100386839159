// rtw_sample_kernel.hpp — radiance queries: Raytracer::sample_ray(&ray, rng, depth) -> Color (lib.rs:97-117) for rays
// the caller chooses, the whole path fused in one persistent launch.  sample_kernel<KernelCfg K> is instantiated beside
// path_kernel<COUNT, K> and hit_kernel<K> (make_variant, rtw_variants.hpp), so a scene's radiance queries run the walk
// and feature set its renders run.
//
// It is path_kernel's non-ring branch with the camera taken out: the grid is at most the kernel's resident capacity,
// each wave keeps a pool of ray indices in LDS, refilled by one lane from a global dispenser word `batch` indices per
// atomic, idle lanes take the next indices by ballot + mbcnt rank once regen_min of them wait, and trace_run is
// resumed across iterations under the render's quota16 / leaf16.  A regenerating lane loads its ray (two quads and the
// stream pair) where path_kernel runs start_path; a ray that is not traced (a bad time, a zero stream word, or
// max_depth = 0) is finished there, path_kernel's off-image case, and the wave draws again.  Each segment is
// trace_begin / trace_run, hit_record<K.feat> with the per-primitive shading record, and the materials' one body
// (rtw_dev_shade.hpp: mat_kind, mat_attenuation, mat_direction) that path_kernel calls too, under path_kernel's
// L = T * terminal rules (T * 0, the solid_light shortcut) written out here: the same f32 operations and draw order, so
// a record's colour is the render's sample bit for bit (tests/test_gpu_sample_rays.py).
//
// What it leaves out of path_kernel: StartArgs and the start ring, the LST rows (the path state stays in VGPRs), SHARD
// (one dispenser word), COUNT builds, the sample buffer and reduce_kernel: a finished path writes its 32-byte record at
// the ray's own index.
#pragma once
#include "../../include/rtw.h"
#include "rtw_query_kernel.hpp"

namespace rtw {

struct SampleArgs {
  DevScene scene;
  const void* rays;  // rtw_ray[n], 16-byte aligned
  void* samples;     // rtw_sample[n], 16-byte aligned
  uint32_t n;        // rays of this launch (the host splits a longer array: SAMPLE_LAUNCH_MAX)
  uint32_t max_depth;
  float bg[3];
  float time_lo, time_hi;  // the committed motion range (Flat): a ray outside it is not traced (RTW_SAMPLE_BAD_RAY)
  uint32_t quota16, leaf16, regen_min, batch;  // RenderArgs' (tune_launch)
  uint32_t spill_lanes;                        // RenderArgs::spill_lanes
  int32_t* spill;                              // RenderArgs::spill
  unsigned long long* counters;                // [0] += the launch's segments (RenderArgs::counters)
  unsigned long long* queue;                   // the ray-index dispenser word, zeroed before every launch
  uint32_t* err;                               // RenderArgs::err
};

// a launch's largest ray count: the path state holds a 32-bit ray index, and dispenser values stay below 2^32
constexpr uint64_t SAMPLE_LAUNCH_MAX = 1ull << 31;

namespace dev {

static_assert(sizeof(rtw_sample) == 32, "rtw_sample layout (include/rtw.h)");

// Every family keeps K.occ, the render's waves per SIMD.  (The 7-wave S16 mesh walk holds its path state in LDS rows in
// path_kernel; here it is in VGPRs and 56 B per lane go to scratch instead, at which it still runs level with its
// render: DESIGN.md §4 lists each family's figures.)
template <KernelCfg K>
__global__ __launch_bounds__(K.blk) __attribute__((amdgpu_waves_per_eu(K.occ, 8))) void sample_kernel(SampleArgs a) {
  // path_kernel's LDS without the LST rows, StartArgs and the ring: the stack columns (+ 1: trace_run's branch-free
  // push), the node table and the waves' index pools
  __shared__ int32_t stk_all[K.stk_words()];
  __shared__ uint16_t stk16_all[K.stk16_words()];
  __shared__ float4 nodes_lds[K.lds_node_quads()];
  fill_nodes_lds<K>(a.scene, nodes_lds);
  // the wave's index pool [next, end) and the batch lane 0 took (path_kernel's pool_lds)
  __shared__ uint64_t pool_lds[K.blk / 64][3];
  uint64_t* const pool = pool_lds[threadIdx.x >> 6];
  const uint32_t lane = threadIdx.x & 63u;
  if (lane == 0) { pool[0] = 0; pool[1] = 0; }
  __syncthreads();
  uint16_t* stk16 = stk16_all + threadIdx.x;
  int32_t* stk = stk_all + threadIdx.x;
  int32_t* spill = a.spill + (size_t)blockIdx.x * K.blk + threadIdx.x;  // unused unless the variant spills
  const DevScene& S = a.scene;
  const V3 bg = ld3(a.bg);
  const uint64_t P = a.n;
  unsigned long long* const dispenser = a.queue;
  const uint32_t batch = a.batch;
  uint32_t cnt[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // (COUNT builds only: never touched here)
  uint64_t ph[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long nrays = 0;
  bool exhausted = false;  // wave-uniform
  bool has = false;
  TraceState ts;
  ts.on = false;
  PathState st;  // pid: the ray's index in this launch; depth: max_depth - the segments that scattered
  st.pid = 0;
  st.rng = 0;
  st.depth = 0;
  // one record, two 16-byte stores at the ray's own index
  auto store = [&](uint32_t idx, V3 L, uint32_t segments, uint64_t word, uint32_t flags) {
    float4* sp = reinterpret_cast<float4*>(reinterpret_cast<char*>(a.samples) + (uint64_t)idx * sizeof(rtw_sample));
    sp[0] = make_float4(L.x, L.y, L.z, __uint_as_float(segments));
    sp[1] = make_float4(__uint_as_float((uint32_t)word), __uint_as_float((uint32_t)(word >> 32)),
                        __uint_as_float(flags), __uint_as_float(0u));
  };
  for (;;) {
    // ---- regeneration: compact new ray indices into the idle lanes
    const uint64_t need = __ballot(!has);
    if (need != 0 && !exhausted && ((uint32_t)__popcll(need) >= a.regen_min || need == __ballot(1))) {
      const uint32_t n_need = (uint32_t)__popcll(need);
      const uint32_t rank =
          __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
      uint64_t pool_next = rfl64(pool[0]), pool_end = rfl64(pool[1]);
      const uint64_t avail = pool_end - pool_next;
      uint64_t nb = P, ne = P;
      if (avail < n_need) {  // refill: one atomic per `batch` rays; lane 0 hands them to the wave through LDS
        if (lane == 0) pool[2] = atomicAdd(dispenser, (unsigned long long)batch);
        const uint64_t b = rfl64(pool[2]);
        if (b < P) {
          nb = b;
          ne = b + batch < P ? b + batch : P;
        } else {
          exhausted = true;
        }
      }
      if (!has) {
        const uint64_t id = rank < avail ? pool_next + rank : nb + (rank - avail);
        if (rank < avail || id < ne) {
          const uint64_t word = load_ray(a.rays, id, st.ray);
          // The caller supplies the generator state and the materials' rejection loops are unbounded: xoroshiro64*
          // never leaves state 0, so the state is mended before anything can draw from it (scatter_kernel's rule; a
          // zero word is marked BAD besides)
          st.rng = xoro_seed(word);
          st.T = mk(1.f, 1.f, 1.f);
          st.depth = a.max_depth;
          st.pid = (uint32_t)id;
          // the BVH's moving-sphere boxes bound [time_lo, time_hi] only: a NaN time fails both compares
          const bool bad = word == 0ull || !(st.ray.time >= a.time_lo && st.ray.time <= a.time_hi);
          if (bad) store(st.pid, mk(0.f, 0.f, 0.f), 0u, 0ull, (uint32_t)RTW_SAMPLE_BAD_RAY);
          else if (a.max_depth == 0u) store(st.pid, mk(0.f, 0.f, 0.f), 0u, word, 0u);  // lib.rs:98-100
          else has = true;
        }
      }
      if (avail >= n_need) {
        pool_next += n_need;
      } else {
        pool_next = nb + (n_need - avail);
        pool_end = ne;
        if (pool_next > pool_end) pool_next = pool_end;
      }
      if (lane == 0) { pool[0] = pool_next; pool[1] = pool_end; }
    }
    if (__ballot(has) == 0) {
      if (exhausted) break;
      continue;  // every ray handed out this round was finished at once: draw again
    }
    // segments starting now, counted per wave with every lane active (so the count is uniform and stays in SGPRs)
    nrays += (unsigned long long)__popcll(__ballot(has && !ts.on));
    if (!has) continue;
    // ---- one segment: closest hit (resumable) + shading (lib.rs:97-117)
    if (!ts.on) {
      trace_begin<false, K.feat, K.stack, K.blk, K.codes16_stack(), K.far_lds_nodes()>(S, st.ray, ts, cnt, st.rng, stk16,
                                                                                       stk, a.err, nodes_lds);
    }
    if (!(K.feat & F_LIST)) {
      const uint32_t act = (uint32_t)__popcll(__ballot(1));
      const uint32_t quota = (act * a.quota16 + 15u) >> 4;
      const uint32_t leaf_thr = (act * a.leaf16 + 15u) >> 4;
      trace_run<false, K.stack, K.spill, K.feat, K.blk, K.ncap, K.half, K.s16>(S, st.ray, ts, stk, spill, a.spill_lanes, cnt,
                                                                              quota, leaf_thr, st.rng, a.err, ph + 4, nodes_lds, stk16);
    } else {
      ts.node = -1;  // list mode: trace_begin tested every primitive
      ts.sp = 0;
    }
    __builtin_amdgcn_s_setprio(0);  // trace_run raised it
    if (ts.node >= 0 || ts.sp > 0) continue;  // traversal suspended: resume next iteration
    ts.on = false;
    const Best b = ts.b;
    bool done = false;
    uint32_t end = 0u;
    V3 L = mk(0.f, 0.f, 0.f);
    const V3 T0 = st.T;
    if (b.prim < 0) {  // lib.rs:102-105
      L = mul(T0, bg);
      done = true;
      end = (uint32_t)RTW_SAMPLE_END_MISS;
      if (__builtin_expect(b.prim == -2, 0)) {
        // trace_run tripped its guard (a corrupt tree; the call reports RTW_EINVAL and its records are invalid): close
        // the dispenser for every wave and empty this wave's pool, so the grid drains after about one trip per wave
        atomicMax(dispenser, (unsigned long long)P);
        pool[0] = pool[1];
        end = (uint32_t)RTW_SAMPLE_BAD_RAY;
      }
    } else {
      const DevShade sh = S.shade[b.prim];
      // a light of one solid colour needs no hit record (path_kernel; mesh kernels only)
      const bool solid_light = (K.feat & F_LIGHT) && (K.feat & F_TRI) && (sh.kind & 0xfffu) == (MT_LIGHT | (SM_SOLID << 8));
      Rec h;
      if (!solid_light) h = hit_record<K.feat>(S, st.ray, b, sh.kind);
      else h = Rec{mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 0.f), 0.0f, 0.0f, true, 0u};
      // the materials' one body (rtw_dev_shade.hpp), the rejection draw and unit() between its pieces
      const MatKind kind = mat_kind<K.feat>(sh.kind);
      V3 rs = mk(0.f, 0.f, 0.f);
      if (kind.lam || kind.met || kind.iso) rs = rand_in_unit_sphere<K.alignbit_draws()>(st.rng);  // vec3.rs:101-108
      const V3 ud = unit(kind.lam ? rs : st.ray.d);  // Lambertian: unit(rs); else unit(d_in)
      const V3 att = mat_attenuation<K.feat>(S, sh, kind, h, [&] { return ld3(sh.b); });
      V3 Tn = mk(0.f, 0.f, 0.f);  // the throughput after this segment (scattering materials)
      if (kind.light) {  // emit, no scatter
        L = mul(T0, att);
        done = true;
        end = (uint32_t)RTW_SAMPLE_END_NO_SCATTER;
      } else {
        const V3 dir = mat_direction<K.feat>(sh, kind, h, ud, rs, st.rng, done);  // done: absorbed
        const V3 T2 = mul(T0, att);  // x * 1.0f == x: the Dielectric's T is unchanged
        // an absorbed Metal ray returns emitted() = black, which the recursion's parents multiply by their
        // attenuations: T * 0, not a constant 0 (path_kernel)
        if (done) {
          L = mul(T0, mk(0.f, 0.f, 0.f));
          end = (uint32_t)RTW_SAMPLE_END_NO_SCATTER;
        }
        Tn = T2;
        st.T = T2;
        st.ray.o = h.p;
        st.ray.d = dir;
      }
      if (!done) {  // lib.rs:98-100: depth 0 returns black, times the attenuations above it (T * 0, as above)
        done = --st.depth == 0u;
        if (done) {
          L = mul(Tn, mk(0.f, 0.f, 0.f));
          end = (uint32_t)RTW_SAMPLE_END_DEPTH;
        }
      }
    }
    if (done) {
      // world.hit queries of the path: one per scattering segment (each took one off depth), and the terminal one
      // unless the path ended because depth ran out
      const uint32_t segments = a.max_depth - st.depth + (end == (uint32_t)RTW_SAMPLE_END_DEPTH ? 0u : 1u);
      if (end == (uint32_t)RTW_SAMPLE_BAD_RAY) store(st.pid, mk(0.f, 0.f, 0.f), 0u, 0ull, end);
      else store(st.pid, L, segments, st.rng, end);
      has = false;
    }
  }
  if (lane == 0 && nrays) atomicAdd(a.counters, nrays);  // nrays counts the whole wave's segments
}

}  // namespace dev
}  // namespace rtw
