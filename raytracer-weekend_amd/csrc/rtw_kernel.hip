// rtw_kernel.hip — what of the gfx950 path-tracing megakernel's host side needs the device compiler: the kernels
// that are no templates (reduce_kernel, unpack_tiles_kernel, tile_list_kernel with its diagnostic calls, the libm and
// reciprocal diagnostics, with the two calls that launch the latter), the tuning knobs, pick_kernel (which path-kernel variant a scene runs) and the launches
// (enqueue_render, enqueue_render_samples, enqueue_tonemap, enqueue_tile_noise, enqueue_tonemap_tiles, enqueue_hit_rays,
// enqueue_occluded_rays, enqueue_sample_rays, enqueue_scatter_rays, enqueue_camera_rays, enqueue_features, enqueue_denoise, enqueue_temporal, enqueue_unpack),
// which share one cache of resident grids (resident_blocks), the walk's tuning (tune_walk) and the one-record-per-lane
// queries' launch (launch_query).  The
// scene's device copies, statistics and the render entry points are plain HIP runtime code in rtw_render.cpp, the
// ray-query entry points in rtw_query.cpp.  The device code is in headers that this unit and rtw_kernel_mesh.hip (the
// F_MESHES variants, under their own compiler flags) both include.
//
// Hot path restated (reference raytracer_weekend_lib/src/):
//   Raytracer::render / sample_pixel (lib.rs:57-95)   -> one work unit per path (pixel, sample); the samples
//                                                        of a pixel are summed in sample order afterwards
//                                                        (rtw_path_kernel.hpp; reduce_kernel here)
//   sample_ray (lib.rs:97-117)                          -> iterative bounce loop, L = T * terminal
//                                                        (rtw_path_kernel.hpp path_kernel)
//   [Box<dyn Hittable>]::hit (hittable/mod.rs:57-69)    -> 4-wide BVH walk (or the flat list), min t,
//                                                        ties -> the larger DFS key (rtw_dev_trace.hpp over
//                                                        rtw_dev_hit.hpp's primitive tests)
//   Material::scatter / emitted (material.rs, light_source.rs) -> the materials' one body, Texture::value
//   (texture.rs, image_texture.rs) and the hit record -> rtw_dev_shade.hpp; Camera::get_ray (camera.rs:66-74) ->
//   start_path (rtw_path_kernel.hpp); the f32 arithmetic and the RNG under all of them -> rtw_dev_math.hpp
//
// Numerics: compiled with -ffp-contract=off and IEEE div/sqrt (hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt), so every primitive test, scatter and the
// throughput product are bit-identical to the oracle's iterative integrator.  Divisions that
// share a divisor use Markstein's correction from an exact reciprocal (rcp_rn, proven over every
// float on the device).  Only the BVH culling uses FMA / rcp approximations, and it is
// conservative (padded boxes + slack), so it changes which nodes are visited, never the answer.
//
// Kernel structure: path_kernel is PERSISTENT -- the grid is the resident capacity,
// and each wave draws path ids from a global queue (RenderArgs::batch per atomic: 1024 in the
// 1024-lane LDS-node and the list-mode kernels, 2048 elsewhere; knob RTW_BATCH) into an LDS pool, hands
// them to its idle lanes by ballot + mbcnt prefix (64 consecutive ids = one sample of one 8x8 tile), and
// loops: regenerate -> trace_begin (the always-tested list) -> trace_run (resumable BVH4 walk with
// postponed leaves; returns once quota16/16 of the lanes are done) -> shade.  A finished path writes
// its radiance to an ordered sample buffer that reduce_kernel sums per pixel in sample order.
// Ray queries (rtw_hit_rays*): hit_kernel<K> (rtw_query_kernel.hpp) runs caller rays through the same trace_begin /
// trace_run / hit_record under the scene's own K, one ray per lane, grid-stride; instantiated beside path_kernel<.., K>.
// Occlusion queries (rtw_occluded_rays*): occluded_kernel<K> (rtw_occluded_kernel.hpp), hit_kernel's shape around an
// any-hit walk to the caller's t_max (trace_run<.., ANY>), one byte per ray.
// Radiance queries (rtw_sample_rays*): sample_kernel<K> (rtw_sample_kernel.hpp) is path_kernel's persistent loop over
// caller rays -- index pool, ballot + mbcnt regeneration, resumable trace_run, the shading body -- without the camera,
// the start ring and the sample buffer: one 32-byte record per ray.  Instantiated beside path_kernel<.., K> as well.
// Scatter and camera-ray queries (rtw_scatter_rays*, rtw_camera_rays*): scatter_kernel and camera_rays_kernel
// (rtw_shade_kernel.hpp) run the materials' body and restate start_path over record arrays; one instantiation each, this
// unit only.
// Progressive renders (rtw_render_samples_device, rtw_render_progressive): a range of samples runs as aligned
// power-of-two blocks, each an ordinary round of passes whose key carries the block's base (frame_args), reduced by
// accumulate_kernel (rtw_film_kernel.hpp) onto the sums the frame holds; tonemap_kernel beside it (rtw_tonemap_device).
// Adaptive renders (rtw_tile_noise_device, rtw_render_adaptive*): tile_noise_kernel and compact_tiles_kernel of the same
// header turn the two sums into the ids of the tiles still above the threshold (enqueue_tile_noise); the loop around
// enqueue_render_samples and it is rtw_render.cpp's.
// The denoiser (rtw_denoise_device): rtw_denoise_kernel.hpp's prepare, a-trous and finish kernels over the film's sums
// and the feature buffers, enqueue_denoise; no scene, no device copy.
// Temporal accumulation (rtw_temporal_device): rtw_temporal_kernel.hpp's one kernel reprojects the history's
// accumulated sums onto the current camera and adds them to the frame's, enqueue_temporal; no scene, no scratch.
// Variants: path_kernel<COUNT, KernelCfg K> -- one plain aggregate (stack rows, spill, waves / SIMD, feature set,
// workgroup size, LDS node table, half nodes, 16-bit stack) is the template argument, defines every property derived
// from it, and travels with the kernel to the host (Variant, rtw_variants.hpp), which sizes the launch from it.
// pick_kernel names the configurations: feature-specialised instantiations; the LDS-node kernel for sphere worlds whose
// tree fits (the whole node table in LDS, sorted-push walk over 16-bit child codes; by default 1024-lane
// workgroups, 2 per CU at 8 waves/SIMD, with the waves' start rings in LDS: DESIGN.md §3); the
// global-node kernels (256-lane workgroups, 32-bit LDS stack) for meshes, with half-precision nodes
// (DevNode4h) for large trees; BVH-less list-mode kernels for <= 32 primitives.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/rtw.h"
#include "rtw_scene.hpp"
#include "rtw_variants.hpp"
#include "rtw_shade_kernel.hpp"
#include "rtw_film_kernel.hpp"
#include "rtw_denoise_kernel.hpp"
#include "rtw_temporal_kernel.hpp"
#include "rtw_tile_beam.h"

namespace rtw {
namespace dev {

// Σ over samples in sample order (lib.rs:83-87), one thread per pixel of the pass.
__global__ __launch_bounds__(256) void reduce_kernel(RenderArgs a, uint32_t n_slots) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_slots * 64u) return;
  const uint32_t slot = g >> 6, l = g & 63u, gslot = a.slot_base + slot;
  const uint32_t tile = a.tile_ids ? a.tile_ids[gslot] : a.tile_first + gslot * a.tile_stride;
  const uint32_t i = (tile % a.tiles_x) * 8u + (l & 7u), row = (tile / a.tiles_x) * 8u + (l >> 3);
  if (i >= a.w || row >= a.h) return;
  float x = 0.f, y = 0.f, z = 0.f;
  const float* q = a.sbuf + ((size_t)slot * a.spp * 64u + l) * 3u;
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
  float* o = a.packed_out ? a.out + ((size_t)gslot * 64u + l) * 3u : a.out + ((size_t)row * a.w + i) * 3u;
  o[0] = x;
  o[1] = y;
  o[2] = z;
}

__global__ void unpack_tiles_kernel(uint32_t w, uint32_t h, uint32_t tiles_x, const uint32_t* tiles,
                                    uint32_t n_tiles, const float* packed, float* img) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_tiles * 64u) return;
  const uint32_t t = g >> 6, lane = g & 63u, tile = tiles[t];
  const uint32_t i = (tile % tiles_x) * 8u + (lane & 7u), row = (tile / tiles_x) * 8u + (lane >> 3);
  if (i >= w || row >= h) return;
  for (int c = 0; c < 3; ++c) img[((size_t)row * w + i) * 3 + c] = packed[(size_t)g * 3 + c];
}

// The per-tile lists of camera rays (path_kernel's ring, K.ldsn_ring()): one thread per 8x8 tile of the
// frame, global tile id = thread id.  The workgroup brings the BVH primitives' padded boxes into the camera's frame
// TILE_LIST_CHUNK at a time (LDS), then every thread runs the beam test of its tile against them in index order and
// keeps the candidates: a 32-B record per tile (TILE_LIST_WORDS), TILE_LIST_OVER past `cap` candidates.  n_over counts
// the tiles on overflow.
constexpr uint32_t TILE_LIST_BLOCK = 64, TILE_LIST_CHUNK = 256;
struct TileListArgs {
  DevCamera cam;
  uint32_t w, h, n_tiles, n_bvh, cap;
  const float4* boxes;  // per BVH prim (lo, 0), (hi, 0)
  uint32_t* lists;
  uint32_t* n_over;
};
__global__ __launch_bounds__(TILE_LIST_BLOCK) void tile_list_kernel(TileListArgs a) {
  __shared__ BeamBox cbox[TILE_LIST_CHUNK];
  const uint32_t tile = blockIdx.x * TILE_LIST_BLOCK + threadIdx.x;
  const BeamCamera C = beam_camera(a.cam.origin, a.cam.u, a.cam.v, a.cam.llc, a.cam.horizontal, a.cam.vertical,
                                   a.cam.lens_radius);
  const BeamTile T = beam_tile(C, a.w, a.h, tile < a.n_tiles ? tile : 0u);
  uint32_t rec[TILE_LIST_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t n = 0;
  for (uint32_t base = 0; base < a.n_bvh; base += TILE_LIST_CHUNK) {
    const uint32_t m = min(TILE_LIST_CHUNK, a.n_bvh - base);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < m; k += TILE_LIST_BLOCK) {
      const float4 lo = a.boxes[2u * (base + k)], hi = a.boxes[2u * (base + k) + 1u];
      const float l[3] = {lo.x, lo.y, lo.z}, h[3] = {hi.x, hi.y, hi.z};
      cbox[k] = beam_box(C, l, h);
    }
    __syncthreads();
    for (uint32_t k = 0; k < m; ++k) {
      if (beam_may_hit(C, T, cbox[k])) {
        ++n;  // halfword n of the record (while it fits)
        if (n <= TILE_LIST_MAX) {
          const uint32_t v = (base + k) << ((n & 1u) * 16u);
#pragma unroll
          for (uint32_t q = 0; q < TILE_LIST_WORDS; ++q) rec[q] |= (n >> 1) == q ? v : 0u;
        }
      }
    }
  }
  if (tile >= a.n_tiles) return;
  const bool over = n > a.cap;
  rec[0] = over ? TILE_LIST_OVER : (rec[0] | n);
  uint4* o = reinterpret_cast<uint4*>(a.lists + (size_t)tile * TILE_LIST_WORDS);
  o[0] = make_uint4(rec[0], rec[1], rec[2], rec[3]);
  o[1] = make_uint4(rec[4], rec[5], rec[6], rec[7]);
  if (over) atomicAdd(a.n_over, 1u);
}

// Diagnostics (rtw_diag_libm): the render path's f32 transcendentals over arrays.
__global__ void libm_kernel(int fn, uint32_t n, const float* a, const float* b, float* out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const float x = a[g];
  if (fn == 4) {  // the camera division: Markstein's correction from the IEEE reciprocal (= RN(1 / b))
    out[g] = div_by_recip(x, b[g], 1.0f / b[g]);
    return;
  }
  if (fn == 5) {  // the sphere test's sqrt
    out[g] = sqrt_rn(x);
    return;
  }
  out[g] = fn == 0 ? dev_log10f(x) : (fn == 1 ? dev_sinf(x) : (fn == 2 ? dev_acosf(x) : dev_atan2f(x, b[g])));
}

// Diagnostics (rtw_diag_sweep): every 32-bit pattern in [lo, hi] as a float b, compared bit for bit
// (NaN == NaN) against the IEEE operation.  fn 0: rcp_rn_fast(b) vs 1.0f / b over the range rcp_rn_ok
// accepts (others are skipped: counted in n[1]).  n[0] = mismatches; the first `cap` are recorded.
__global__ void sweep_kernel(int fn, uint32_t lo, uint32_t hi, unsigned long long* n, uint32_t* bad, uint32_t cap) {
  const uint64_t span = (uint64_t)hi - lo + 1u;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long nbad = 0, nskip = 0;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < span; k += stride) {
    const uint32_t bits = lo + (uint32_t)k;
    const float b = __uint_as_float(bits);
    bool ok = true;
    if (fn == 0) {
      if (!rcp_rn_ok(b)) {
        ++nskip;
        continue;
      }
      const float f = rcp_rn_fast(b), r = 1.0f / b;
      ok = __float_as_uint(f) == __float_as_uint(r) || (f != f && r != r);
    }
    if (!ok) {
      const unsigned long long slot = atomicAdd(n + 2, 1ull);
      if (slot < cap) bad[slot] = bits;
      ++nbad;
    }
  }
  if (nbad) atomicAdd(n, nbad);
  if (nskip) atomicAdd(n + 1, nskip);
}

}  // namespace dev

// ---------------------------------------------------------------- host side
// Paths per pass (ordered sample buffer = 12 B per path): 2^32 = 51.5 GB of the 288 GB HBM.  A frame
// with more paths (monument 4K x 1024 spp: 8.5 G, 2 passes) runs in several passes, each one persistent
// launch + its in-order reduction.  Tuning knob RTW_PASS_LOG2 (24..33).
static uint64_t max_pass_paths(const Knobs& kn) {
  return 1ull << std::min(32, std::max(24, kn.pass_log2.get(32)));  // PathState::pid is 32-bit
}

// Every tuning knob of this file, read here and nowhere else (RTW_VERBOSE only prints: it needs no RTW_TUNING gate)
static Knobs read_knobs() {
  auto knob = [](const char* name) {
    const char* e = tuning_env(name);
    return e ? Knob{true, atoi(e)} : Knob{};
  };
  Knobs k;
  k.stack_lds = knob("RTW_STACK_LDS");
  k.half_nodes = knob("RTW_HALF_NODES");
  k.generic = knob("RTW_GENERIC");
  k.list_all = knob("RTW_LIST_ALL");
  k.list_occ = knob("RTW_LIST_OCC");
  k.occ = knob("RTW_OCC");
  k.ldsn_waves = knob("RTW_LDSN_WAVES");
  k.lds_nodes = knob("RTW_LDS_NODES");
  k.ldsn_blk = knob("RTW_LDSN_BLK");
  k.mesh_s16 = knob("RTW_MESH_S16");
  k.batch = knob("RTW_BATCH");
  k.quota16 = knob("RTW_QUOTA16");
  k.leaf16 = knob("RTW_LEAF16");
  k.regen_min = knob("RTW_REGEN_MIN");
  k.pass_log2 = knob("RTW_PASS_LOG2");
  k.tile_lists = knob("RTW_TILE_LISTS");
  k.tile_list_cap = knob("RTW_TILE_LIST_CAP");
  const char* v = getenv("RTW_VERBOSE");
  k.verbose = v && atoi(v);
  return k;
}

// Variants of the path kernel: feature set x the waves per SIMD the register allocator must allow.
// Sphere-only scenes (jumpy-balls) get the specialised kernel; everything else the generic one.
// Trees whose push bound exceeds the LDS stack get the SPILL variant.  Default: 5 waves/SIMD.
// Tuning knobs: RTW_OCC=4 (33-row stack) or RTW_OCC=6 (specialised kernel; spills registers);
// RTW_STACK_LDS=4 selects a generic kernel with a 4-entry LDS stack, so that the HBM spill path
// runs on every scene (tests/test_gpu_parity.py).
static Variant pick_kernel(const Knobs& kn, uint32_t feat, uint32_t need, bool list, uint32_t n_nodes, uint32_t need4,
                           bool codes16, bool has_half, bool far) {
  using namespace dev;
  if (kn.stack_lds.get(0) == 4) return make_variant<SPILL_TEST>();  // spill-path test
  const bool sph = (feat & ~F_SPHERES) == 0;
  // Half-precision nodes (DevNode4h, built when the 16-bit codes fit) trade vector-memory traffic (4 loads /
  // 64 B per visit instead of 7 / 112 B) for VALU issue (v_fma_mix_f32 issues ~1.3x slower than v_fma_f32,
  // scripts/ubench/mix_rate.hip; +5 VALU per visit).  Measured (profiles/r03/experiments, h1): monument-4k
  // +3.3% (its 2,226-node tree), cow-1080p -6.5% (1,591 nodes), jumpy-1080p -4.9% (LDS nodes) at round 3's 5-wave
  // mesh kernel.  With round 4's 6-wave mesh walk (16-bit stack, LDS state rows; pick5) the cow gains too (r04q:
  // +1.8%), so every mesh tree with a half table uses it by default; the LDS-node sphere kernels keep f32 nodes.
  // Knob RTW_HALF_NODES 1 = wherever built (LDS-node kernels too), 0 = never.
  const int half_knob = kn.half_nodes.get(-1);
  // (no half-precision table when a bound is beyond f16's range: rtw_flatten.cpp half_node)
  const bool half = has_half && half_knob != 0;
  const bool half_lds = has_half && half_knob > 0;
  if (list) {
    // RTW_GENERIC on a list world: the all-features LIST kernel, whose fold is the reference's (NaN candidates, list
    // order); the BVH kernels' fold treats a NaN candidate as a miss
    if (kn.generic.get(0)) return make_variant<LIST_ALL>();
    // The rect/instance list kernel needs 56 VGPRs and runs at 8 waves/SIMD (cornell-box on MI355X: 26.7k Mrays/s
    // at 5-6 waves, 28.9k at 7, 29.5k at 8; knob RTW_LIST_OCC); the all-features one spills below 96 VGPRs, so
    // it stays at 5.
    if ((feat & ~F_BOXES) == 0 && !kn.list_all.get(0)) {  // knob: the all-features list kernel instead
      if (kn.list_occ.get(8) == 6) return make_variant<LIST_BOXES6>();
      return make_variant<LIST_BOXES8>();
    }
    return make_variant<LIST_ALL>();
  }
  // sphere worlds default to 6 waves/SIMD (24 B/lane of register spill, +1.6% on jumpy-balls over
  // 5 waves once the kernel-uniform values left the VGPRs); the other variants to 5
  switch (kn.occ.get(sph ? 6 : 5)) {
    case 4: {
      const bool sp = need > (uint32_t)STACK_LDS;
      if (sph) return sp ? make_variant<with_spill(WALK4<F_SPHERES>)>() : make_variant<WALK4<F_SPHERES>>();
      return sp ? make_variant<with_spill(WALK4<F_ALL>)>() : make_variant<WALK4<F_ALL>>();
    }
    case 6: {
      // the LDS-node kernels (see their configurations): a sphere world whose sorted-push stack bound and node
      // table fit the variant's rows and capacity
      const int ldsn_waves = kn.ldsn_waves.get(8);
      const bool ldsn = sph && codes16 && kn.lds_nodes.get(1);
      auto fits = [&](const KernelCfg& k) { return need4 <= (uint32_t)k.stack && n_nodes <= (uint32_t)k.ncap; };
      if (ldsn && ldsn_waves == 7 && fits(LDSN_448))
        return half_lds ? make_variant<with_half(LDSN_448)>() : make_variant<LDSN_448>();
      if (ldsn && ldsn_waves == 8 && fits(LDSN_1024) && !half_lds && kn.ldsn_blk.get(1024) == 1024)
        return make_variant<LDSN_1024>();
      if (ldsn && ldsn_waves == 8 && fits(LDSN_512))
        return half_lds ? make_variant<with_half(LDSN_512)>() : make_variant<LDSN_512>();
      if (ldsn && fits(LDSN_224))
        return half_lds ? make_variant<with_half(LDSN_224)>() : make_variant<LDSN_224>();
      if (sph && need <= (uint32_t)STACK_LDS5) return make_variant<SPHERES6>();
    }
      [[fallthrough]];
    default:
      if (kn.generic.get(0)) return pick5<F_ALL>(kn, need);  // parity of the generic kernel
      if (sph) return pick5<F_SPHERES>(kn, need);
      if ((feat & ~F_BOXES) == 0) return pick5<F_BOXES>(kn, need);
      if ((feat & ~F_SMOKE) == 0) return pick5<F_SMOKE>(kn, need);
      if ((feat & ~F_MESHES) == 0) {
        // a partial LDS node cache (the top 128 / 376 / 760 node4s, the rest from global memory, sorted-push
        // walk) measured slower on cow / monument (profiles/r02/experiments, n7): the full-table kernels
        // are for trees that fit
        if (far) return pick5<F_ALL>(kn, need);  // spheres in a mesh world's BVH: the mesh kernels have no far path
        return pick_mesh(kn, need, half, codes16);
      }
      return pick5<F_ALL>(kn, need);
  }
}
static Variant path_kernel_variant(const Flat& f, const Knobs& kn) {
  const uint32_t feat = f.features, need = f.stack_need, need4 = f.stack_need4, nn = (uint32_t)f.nodes4.size();
  const bool list = f.nodes4.empty();
  const bool hh = f.codes16 && !f.nodes4h.empty();
  return pick_kernel(kn, feat, need, list, nn, need4, f.codes16, hh, f.far_check != 0);
}

// rtw_scene_info 16-23: the configuration of the path kernel the current environment selects for the committed
// scene.  Host only: no device is touched.
int64_t selected_kernel_info(const Scene& s, int field) {
  const KernelCfg k = path_kernel_variant(s.flat, read_knobs()).cfg;
  const int64_t v[8] = {k.stack, k.spill, k.occ, k.feat, k.blk, k.ncap, k.half, k.s16};
  return field >= 0 && field < 8 ? v[field] : -1;
}

// rtw_scene_info 24, 25: whether the last render on the scene's first device copy resolved its camera rays from tile
// lists, and how many of the frame's tiles were on overflow (waits for that render)
int64_t last_render_lists(Scene& s, int field) {
  DeviceCopy* c = find_copy(s, -1);
  if (!c) return 0;
  if (field == 0 || !c->lists_used) return field == 0 ? (int64_t)c->lists_used : 0;
  DeviceGuard g;
  uint32_t n = 0;
  if (hipSetDevice(c->phys) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(&n, c->lists_count, sizeof n, hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  return (int64_t)n;
}

// The resident capacity of kernel fn in blocks of `block` lanes on c's device (blocks per CU x CUs): the persistent
// path kernel's grid and the largest grid of a query kernel.  Computed at first use and when a knob switched the
// slot's kernel.
static int resident_blocks(DeviceCopy& c, GridSlot slot, const void* fn, int block, const char* what, bool verbose) {
  ResidentGrid& g = c.grids[slot];
  if (g.blocks > 0 && g.fn == fn) return g.blocks;
  int per_cu = 0, cus = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, block, 0);
  if (e != hipSuccess || per_cu < 1) per_cu = 1;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c.phys) != hipSuccess || cus < 1) cus = 256;
  g = ResidentGrid{fn, per_cu * cus};
  if (verbose)
    fprintf(stderr, "rtw: %s %p: block %d, %d resident blocks per CU x %d CUs\n", what, fn, block, per_cu, cus);
  return g.blocks;
}

// A query kernel over n records, one per lane, between ev0 and ev1 (or NULL): at most `resident` blocks (the kernels
// stride by the grid beyond them), none for n = 0
template <class Kernel, class Args>
static int launch_query(Kernel kernel, const char* what, int resident, int block, uint64_t n, const Args& a,
                        hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  const int grid = (int)std::min<uint64_t>((uint64_t)resident, (n + (uint32_t)block - 1u) / (uint32_t)block);
  if (ev0) HIPCHK(hipEventRecord(ev0, stream), "hipEventRecord");
  if (grid > 0) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, a);
    HIPCHK(hipGetLastError(), what);
  }
  if (ev1) HIPCHK(hipEventRecord(ev1, stream), "hipEventRecord");
  return RTW_OK;
}

// A batch size (knob RTW_BATCH) as the kernels take it: within [64, 65536] and rounded down to a multiple of 64.
// Passes hold 64 x spp ids per slot, so every batch of a pass, its last one included, is then whole groups of 64
// consecutive ids: path_kernel's start ring (SRING) builds 64 starts from pool_next + lane without a bound check.
static uint32_t batch_ids(int v) { return (uint32_t)std::min(65536, std::max(64, v)) & ~63u; }

// The DISP path-id dispensers (path_kernel; sample_kernel uses the first), DISP_STRIDE words apart, behind the
// counters' 32 statistics words
static unsigned long long* dispensers(const DeviceCopy& c) { return c.counters + 32; }

// enqueue_render, part 1: the RenderArgs of a frame and its tiles, all but the launch tuning.  Pure host arithmetic.
static RenderArgs frame_args(const DeviceCopy& c, const Frame& f, const TileSet& ts, float* d_out) {
  const rtw_camera* cam = f.cam;
  RenderArgs a;
  memset(&a, 0, sizeof a);
  a.scene = c.scene;
  memcpy(a.cam.origin, cam->origin, sizeof a.cam.origin);
  memcpy(a.cam.llc, cam->lower_left_corner, sizeof a.cam.llc);
  memcpy(a.cam.horizontal, cam->horizontal, sizeof a.cam.horizontal);
  memcpy(a.cam.vertical, cam->vertical, sizeof a.cam.vertical);
  memcpy(a.cam.u, cam->u, sizeof a.cam.u);
  memcpy(a.cam.v, cam->v, sizeof a.cam.v);
  a.cam.lens_radius = cam->lens_radius;
  a.cam.time0 = cam->time0;
  a.cam.time1 = cam->time1;
  memcpy(a.bg, f.bg, sizeof a.bg);
  a.w = f.w; a.h = f.h; a.spp = f.spp; a.max_depth = f.max_depth;
  a.tiles_x = f.tiles_x();
  a.spp_magic = f.spp > 1u ? UINT64_MAX / f.spp + 1u : 0u;
  a.fw1 = (float)(f.w - 1u);
  a.fh1 = (float)(f.h - 1u);
  a.rw1 = recip_rn(a.fw1);
  a.rh1 = recip_rn(a.fh1);
  {
    volatile float t0 = cam->time0, t1 = cam->time1;  // one IEEE f32 subtraction, as on the device
    a.time_span = t1 - t0;
  }
  a.tiles_x_magic = a.tiles_x > 1u ? UINT64_MAX / a.tiles_x + 1u : 0u;
  a.tile_ids = ts.ids;
  a.tile_first = ts.first;
  a.tile_stride = ts.stride;
  a.packed_out = ((ts.ids && !ts.full) || ts.packed) ? 1u : 0u;
  a.err = c.err_host;
  // the host mirror of dev::splitmix64 (seed pre-hash shared by every pixel)
  uint64_t z = f.seed + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  // the path key is seed_hash ^ (j << 48 | i << 32 | s) with s < spp (start_path): a block's base, a multiple of its
  // power-of-two spp, joins s here (base ^ s == base + s)
  a.seed_hash = (z ^ (z >> 31)) ^ (uint64_t)f.sample_base;
  a.out = d_out;
  a.counters = c.counters;
  a.queue = dispensers(c);
  return a;
}

// The BVH walk's launch tuning of variant k on `grid` resident workgroups: what a render's path kernel and a query's
// hit kernel share (trace_run)
struct WalkTuning {
  uint32_t leaf16, spill_depth, spill_lanes;
};
static WalkTuning tune_walk(const Knobs& kn, const Flat& flat, const KernelCfg& k, int grid) {
  WalkTuning t;
  // test postponed leaves once leaf16/16 of the wave's lanes hold one and cannot descend (trace_run); knob
  // RTW_LEAF16 (1..16).  The sorted-push walk of the LDS-node kernels parks fewer leaves early: 5/16 measured best
  // on jumpy-balls (+0.5% over 3; profiles/r02/experiments, n5)
  const bool ldsn_spheres = k.lds_nodes() && flat.features == (flat.features & F_SPHERES);
  t.leaf16 = (uint32_t)std::min(16, std::max(1, kn.leaf16.get(ldsn_spheres ? 5 : 3)));
  // the LDS-node variants walk 16-bit codes within their own stack rows (pick_kernel checked
  // stack_need4 against them) and have no HBM spill path
  const uint32_t lds = (uint32_t)k.stack;
  t.spill_depth = (!k.lds_nodes() && flat.stack_need > lds) ? flat.stack_need - lds : 0;
  t.spill_lanes = (uint32_t)grid * (uint32_t)k.blk;
  return t;
}

// The launch tuning of variant k's persistent loop on `grid` resident workgroups: what a render's path kernel
// (enqueue_render, part 2) and a radiance query's sample kernel share.  batch is the full-frame value: pass_batch
// shrinks it for a small pass.
struct LaunchTuning {
  WalkTuning walk;
  uint32_t quota16, regen_min, batch;
};
static LaunchTuning tune_launch(const Knobs& kn, const Flat& flat, const KernelCfg& k, int grid) {
  LaunchTuning a;
  a.walk = tune_walk(kn, flat, k, grid);
  // see trace_run (measured best of 4..16 on jumpy-balls); tuning knob RTW_QUOTA16 (1..16); run_passes lowers it for
  // a full-size pass whose camera rays are resolved from the tile lists
  a.quota16 = (uint32_t)std::min(16, std::max(1, kn.quota16.get(12)));
  // whole wave-loads of ids only (batch_ids): the start ring makes 64 path starts from 64 consecutive ids of a batch.
  // The 1024-lane LDS-node kernel and the BVH-less list kernels: 1024 ids per atomic (a shorter end-of-frame
  // tail; jumpy-1080p +1.2%, cornell-800 +0.5% over 2048, profiles/r03/experiments k3 / k4); the mesh
  // kernels keep 2048 (neutral on cow; their short paths made small batches costly in round 2)
  const bool small_batch = (k.lds_nodes() && k.blk == 1024) || flat.nodes4.empty();
  a.batch = batch_ids(kn.batch.get(small_batch ? 1024 : (int)dev::BATCH));
  // Regenerate paths only once >= regen_min lanes of a wave are idle (or all are): start_path
  // runs at wave level, so batching it raises its SIMD utilisation.  Measured on MI355X
  // (RTW_REGEN_MIN sweep 1..32): 24 is best for open scenes (jumpy-balls +4.3%, cow +1.6%,
  // monument +1.7% over 1); closed boxes (cornell: 6.6 segments per path, few lanes finish per
  // iteration) lose with deep deferral: 8 (cornell list variant at 8 waves/SIMD: 29.3k at 1, 29.4k at 4, 29.8k at 8, 28.1k at 24).
  // With the start ring (round 6, the rect list kernel) a regeneration costs a few LDS reads, not start_path at
  // the idle lanes' occupancy, so waves refill early: REGEN_RING (cornell-800: 8 -> 2, +1.8%).  The 1024-lane
  // sphere kernel's take finishes the start (start_take) and its paths are shorter: REGEN_RING_LDSN
  // (profiles/r07/experiments).
  const bool boxed = (flat.features & ~F_SMOKE) == 0;
  const int regen_dflt = k.ldsn_ring() ? REGEN_RING_LDSN : (k.sring() ? REGEN_RING : (boxed ? 8 : 24));
  a.regen_min = (uint32_t)std::min(64, std::max(1, kn.regen_min.get(regen_dflt)));
  return a;
}

// Small frames: fewer ids per atomic, halving until every resident wave can take >= 32 batches.  configs[0]
// (jumpy-balls 400x225x50: 4.5 M paths for 8,192 resident waves) handed out 4,395 batches of 1,024, so half the
// waves got none and the kernel ran 5x slower per ray than at 1080p: 5.43k -> 9.30k Mrays/s at 128.  The same
// for an 8-GPU share (one eighth of the paths): jumpy +5% at 256, cornell +4.4% at 256, cow +22% at 512
// (profiles/r05/experiments, r05l).  Floors: the mesh / generic kernels' short paths queue on the one atomic
// word below 512 (cow 256: -16%), the others' below 128.  Full frames keep the defaults (>= 32 batches per
// wave already); knob RTW_BATCH sets the size outright.
// (a pass this rule gave smaller batches spreads its atomics over DISP words in the LDS-node kernels:
// path_kernel SHARD; r06 share8: an 8-GPU share of jumpy-1080p +5%, configs[0] +11%)
static uint32_t pass_batch(uint32_t batch0, uint64_t n_paths, uint64_t waves) {
  const uint32_t batch_floor = batch0 >= 2048u ? 512u : 128u;
  uint32_t batch = batch0;
  while (batch / 2u >= batch_floor && n_paths < (uint64_t)batch * waves * 32u) batch /= 2u;
  return batch;
}

// The ordered sample buffer's bytes for passes of `spp` samples over n_slots tiles: the largest pass's paths
static size_t sample_buffer_bytes(const Knobs& kn, uint32_t n_slots, uint32_t spp) {
  const uint64_t per_slot = 64ull * spp;
  const uint64_t slots_per_pass = std::max<uint64_t>(1, max_pass_paths(kn) / per_slot);
  return (size_t)(std::min<uint64_t>(n_slots, slots_per_pass) * per_slot * 3 * sizeof(float));
}

// What a pass's in-order reduction does with the sums: nullptr = reduce_kernel starts them (rtw_render*); a Film =
// accumulate_kernel continues the ones at RenderArgs::out, and the sums of squares at sq when there is one
struct Film {
  float* sq;
};

// enqueue_render, part 3: the pass loop over n_slots tiles, each pass one persistent launch of the scene's variant and
// its in-order reduction
static int run_passes(Scene& sc, DeviceCopy& c, RenderArgs& a, const Knobs& kn, uint32_t n_slots, bool count,
                      hipStream_t stream, const Film* film = nullptr) {
  const uint64_t per_slot = 64ull * a.spp;
  const uint32_t slots_per_pass = (uint32_t)std::max<uint64_t>(1, max_pass_paths(kn) / per_slot);
  // the ordered sample buffer (first render only)
  if (int e = grow(c.sbuf, sample_buffer_bytes(kn, n_slots, a.spp))) return e;
  a.sbuf = static_cast<float*>(c.sbuf.p);
  const Variant var = path_kernel_variant(sc.flat, kn);
  const KernelCfg& k = var.cfg;
  const int grid = resident_blocks(c, count ? GRID_PATH_COUNT : GRID_PATH, (const void*)var.fn[count], k.blk,
                                   "path kernel", kn.verbose);
  const LaunchTuning t = tune_launch(kn, sc.flat, k, grid);
  a.quota16 = t.quota16;
  a.leaf16 = t.walk.leaf16;
  a.regen_min = t.regen_min;
  a.spill_depth = t.walk.spill_depth;
  a.spill_lanes = t.walk.spill_lanes;
  // (first render of a deep tree only)
  if (int e = grow(c.spill, (size_t)a.spill_depth * a.spill_lanes * sizeof(int32_t))) return e;
  a.spill = static_cast<int32_t*>(c.spill.p);
  const uint64_t waves = (uint64_t)grid * (uint32_t)k.blk / 64u;
  for (uint32_t base = 0; base < n_slots; base += slots_per_pass) {
    const uint32_t ns = std::min(slots_per_pass, n_slots - base);
    a.slot_base = base;
    a.n_paths = (uint64_t)ns * per_slot;
    a.batch = kn.batch.set ? t.batch : pass_batch(t.batch, a.n_paths, waves);
    // A pass whose camera rays are resolved from the tile lists walks bounce rays only, which finish further apart,
    // and the quota is a share of the lanes that walk (path_kernel): 8/16 measured best of 4..14 at 1080p, +3% over
    // 12.  A small pass (one pass_batch gave smaller batches: its end-of-pass tail counts) keeps 12: jumpy-400 lost 5%
    // at 8 (profiles/r08/experiments).
    if (!kn.quota16.set) a.quota16 = (a.tile_lists && a.batch == t.batch) ? 8u : t.quota16;
    if (base) HIPCHK(hipMemsetAsync(a.queue, 0, DISP * DISP_STRIDE * sizeof(unsigned long long), stream),
                     "hipMemsetAsync(queue)");
    hipEvent_t* ke = c.kev[c.kev_head];
    if (int e = ensure_event(ke[0])) return e;
    if (int e = ensure_event(ke[1])) return e;
    HIPCHK(hipEventRecord(ke[0], stream), "hipEventRecord");
    hipLaunchKernelGGL(var.fn[count], dim3(grid), dim3(k.blk), 0, stream, a);
    HIPCHK(hipGetLastError(), "path_kernel launch");
    HIPCHK(hipEventRecord(ke[1], stream), "hipEventRecord");
    c.kev_head = (c.kev_head + 1) % 64u;
    c.kev_count = std::min(c.kev_count + 1u, 64u);
    if (film) {
      hipLaunchKernelGGL(dev::accumulate_kernel, dim3((ns * 64u + dev::FILM_BLOCK - 1u) / dev::FILM_BLOCK),
                         dim3(dev::FILM_BLOCK), 0, stream, a, ns, film->sq, film->sq ? 1u : 0u);
      HIPCHK(hipGetLastError(), "accumulate_kernel launch");
    } else {
      hipLaunchKernelGGL(dev::reduce_kernel, dim3((ns * 64u + 255u) / 256u), dim3(256), 0, stream, a, ns);
      HIPCHK(hipGetLastError(), "reduce_kernel launch");
    }
  }
  return RTW_OK;
}

// The per-tile lists serve a render when every camera ray starts from a *near* origin, the ones the BVH's sphere boxes
// are padded for (rtw_flatten.cpp far_bound: D(o) <= D0): D is convex in o, so the four corners of the lens' bounding
// square decide for the whole lens.  In double, with slack for the kernel's f32 origin.
static bool lens_is_near(const Flat& flat, const rtw_camera& cam) {
  if (!flat.far_check) return false;
  const DevFar& F = flat.far;
  const double R = fabs((double)cam.lens_radius);
  for (int q = 0; q < 4; ++q) {
    double D2 = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double o = (double)cam.origin[k] + ((q & 1) ? R : -R) * (double)cam.u[k] + ((q & 2) ? R : -R) * (double)cam.v[k];
      const double t = fabs(o - (double)F.mid[k]) + (double)F.half[k];
      D2 += t * t;
    }
    if (!(D2 * (1.0 + 1.0e-6) <= (double)F.d2)) return false;  // (a NaN camera: off)
  }
  return true;
}

static dev::TileListArgs tile_list_args(const rtw_camera& cam, uint32_t w, uint32_t h, uint32_t n_bvh, uint32_t cap) {
  dev::TileListArgs t;
  memset(&t, 0, sizeof t);
  memcpy(t.cam.origin, cam.origin, sizeof t.cam.origin);
  memcpy(t.cam.llc, cam.lower_left_corner, sizeof t.cam.llc);
  memcpy(t.cam.horizontal, cam.horizontal, sizeof t.cam.horizontal);
  memcpy(t.cam.vertical, cam.vertical, sizeof t.cam.vertical);
  memcpy(t.cam.u, cam.u, sizeof t.cam.u);
  memcpy(t.cam.v, cam.v, sizeof t.cam.v);
  t.cam.lens_radius = cam.lens_radius;
  t.w = w;
  t.h = h;
  t.n_tiles = (uint32_t)(((uint64_t)(w + 7u) / 8u) * ((h + 7u) / 8u));
  t.n_bvh = n_bvh;
  t.cap = cap;
  return t;
}

// Builds the frame's tile records on `stream` into `lists` (TILE_LIST_WORDS per tile of the frame) and zeroes, then
// counts, the tiles on overflow in *n_over.  A render rebuilds them on every call: camera and size change from frame
// to frame in real use, and the build is a few tens of microseconds (profiles/r08/experiments).
static int enqueue_tile_lists(Scene& sc, DeviceCopy& c, const rtw_camera& cam, uint32_t w, uint32_t h, uint32_t cap,
                              uint32_t* lists, uint32_t* n_over, hipStream_t stream) {
  dev::TileListArgs t = tile_list_args(cam, w, h, sc.flat.far.n_bvh, cap);
  t.boxes = static_cast<const float4*>(c.pboxes.p);
  t.lists = lists;
  t.n_over = n_over;
  HIPCHK(hipMemsetAsync(n_over, 0, sizeof(uint32_t), stream), "hipMemsetAsync(tile-list counter)");
  hipLaunchKernelGGL(dev::tile_list_kernel, dim3((t.n_tiles + dev::TILE_LIST_BLOCK - 1u) / dev::TILE_LIST_BLOCK),
                     dim3(dev::TILE_LIST_BLOCK), 0, stream, t);
  HIPCHK(hipGetLastError(), "tile_list_kernel launch");
  return RTW_OK;
}
// whether a render of `cam` resolves its camera rays from tile lists, and the cap it builds them with
static bool tile_lists_on(const Scene& sc, const DeviceCopy& c, const rtw_camera& cam, uint32_t* cap) {
  const Knobs kn = read_knobs();
  *cap = (uint32_t)std::min((int)TILE_LIST_MAX, std::max(1, kn.tile_list_cap.get((int)TILE_LIST_MAX)));
  const uint32_t n_bvh = sc.flat.far.n_bvh;
  return kn.tile_lists.get(1) != 0 && path_kernel_variant(sc.flat, kn).cfg.ldsn_ring() && c.pboxes.p &&
         c.lists_count && n_bvh > 0 && n_bvh < TILE_LIST_OVER && sc.flat.pboxes.size() == (size_t)n_bvh * 8u &&
         lens_is_near(sc.flat, cam);
}

// The frame's tile lists, before its passes (records by global tile id: every tile subset, pass and block of samples
// reads the same table): sets c.lists_used and *lists (NULL when the render does not use them)
static int frame_tile_lists(Scene& sc, DeviceCopy& c, const Frame& f, hipStream_t stream, const uint32_t** lists) {
  uint32_t cap = 0;
  *lists = nullptr;
  c.lists_used = tile_lists_on(sc, c, *f.cam, &cap) ? 1u : 0u;
  if (!c.lists_used) return RTW_OK;
  // (the buffer is grown once, like the sample buffer)
  // The build measured 0.2 ms at 1080p (profiles/r08/experiments), above the 0.1 ms a rebuild per call was
  // allowed: the records are kept for the (camera, size, cap) they were built for, compared field by field, and a
  // render on the same stream with the same ones reuses them (an animation's frames rebuild, a frame's tile
  // subsets, passes and repeats do not)
  DeviceCopy::ListsKey& key = c.lists_key;
  const bool same = key.valid && key.w == f.w && key.h == f.h && key.cap == cap && key.stream == stream &&
                    memcmp(&key.cam, f.cam, sizeof key.cam) == 0;
  if (!same) {
    key.valid = false;
    if (int e = grow(c.tile_lists, (size_t)f.tiles() * TILE_LIST_WORDS * sizeof(uint32_t))) return e;
    if (int e = enqueue_tile_lists(sc, c, *f.cam, f.w, f.h, cap, static_cast<uint32_t*>(c.tile_lists.p),
                                   c.lists_count, stream))
      return e;
    key.cam = *f.cam;
    key.w = f.w; key.h = f.h; key.cap = cap; key.stream = stream;
    key.valid = true;
  }
  *lists = static_cast<const uint32_t*>(c.tile_lists.p);
  return RTW_OK;
}

int enqueue_render(Scene& sc, DeviceCopy& c, const Frame& f, const TileSet& ts, float* d_out, hipStream_t stream,
                   uint32_t flags, hipEvent_t ev0, hipEvent_t ev1) {
  // an earlier render on this device (one the caller did not wait on) tripped the guard: report it now
  if (int e = check_guard(c)) return e;
  if (int e = check_image_max(f.w, f.h)) return e;
  if (int e = check_shutter(*f.cam, sc.flat)) return e;
  RenderArgs a = frame_args(c, f, ts, d_out);
  const Knobs kn = read_knobs();
  c.lists_used = 0;
  HIPCHK(hipMemsetAsync(c.counters, 0, COUNTER_WORDS * sizeof(unsigned long long), stream), "hipMemsetAsync");
  if (ev0) HIPCHK(hipEventRecord(ev0, stream), "hipEventRecord");
  if (ts.n && (f.spp == 0 || f.max_depth == 0)) {  // lib.rs:83 loops 0 times / :98 returns black
    size_t n = a.packed_out ? (size_t)ts.n * 64 * 3 : (size_t)f.w * f.h * 3;
    HIPCHK(hipMemsetAsync(d_out, 0, n * sizeof(float), stream), "hipMemsetAsync(out)");
  } else if (ts.n) {
    if (int e = frame_tile_lists(sc, c, f, stream, &a.tile_lists)) return e;
    if (int e = run_passes(sc, c, a, kn, ts.n, flags & RTW_FLAG_COUNT_TRAVERSAL, stream)) return e;
  }
  if (ev1) HIPCHK(hipEventRecord(ev1, stream), "hipEventRecord");
  return RTW_OK;
}

uint32_t sample_blocks(uint32_t first, uint32_t n, uint32_t* firsts, uint32_t* log2s) {
  uint32_t nb = 0;
  for (uint64_t p = first, end = (uint64_t)first + n; p < end; ++nb) {
    uint32_t k = p ? (uint32_t)__builtin_ctzll(p) : 31u;  // the largest block that may start at p ...
    while ((1ull << k) > end - p) --k;                    // ... and fits what is left
    firsts[nb] = (uint32_t)p;
    log2s[nb] = k;
    p += 1ull << k;
  }
  return nb;
}

int enqueue_render_samples(Scene& sc, DeviceCopy& c, const Frame& f, uint32_t sample_first, const TileSet& ts,
                           float* d_sum, float* d_sq, hipStream_t stream, uint32_t flags, hipEvent_t ev0,
                           hipEvent_t ev1) {
  if (int e = check_guard(c)) return e;
  if (int e = check_image_max(f.w, f.h)) return e;
  if (int e = check_shutter(*f.cam, sc.flat)) return e;
  const Knobs kn = read_knobs();
  c.lists_used = 0;
  HIPCHK(hipMemsetAsync(c.counters, 0, COUNTER_WORDS * sizeof(unsigned long long), stream), "hipMemsetAsync");
  if (ev0) HIPCHK(hipEventRecord(ev0, stream), "hipEventRecord");
  // no sample or no depth: every sample is black (lib.rs:83 / :98), and x + 0 would only turn a -0 into +0
  if (ts.n && f.spp && f.max_depth) {
    uint32_t firsts[SAMPLE_BLOCKS_MAX], log2s[SAMPLE_BLOCKS_MAX];
    const uint32_t nb = sample_blocks(sample_first, f.spp, firsts, log2s);
    const uint32_t* lists = nullptr;
    if (int e = frame_tile_lists(sc, c, f, stream, &lists)) return e;
    // the sample buffer for the largest block, once: no block's run_passes then frees what an earlier one reads
    const uint32_t big = *std::max_element(log2s, log2s + nb);
    if (int e = grow(c.sbuf, sample_buffer_bytes(kn, ts.n, 1u << big))) return e;
    const Film film{d_sq};
    for (uint32_t k = 0; k < nb; ++k) {
      Frame fb = f;
      fb.spp = 1u << log2s[k];
      fb.sample_base = firsts[k];
      RenderArgs a = frame_args(c, fb, ts, d_sum);
      a.tile_lists = lists;
      // (the counters' reset above zeroed the dispensers for the first block; the statistics words run on)
      if (k) HIPCHK(hipMemsetAsync(a.queue, 0, DISP * DISP_STRIDE * sizeof(unsigned long long), stream),
                    "hipMemsetAsync(queue)");
      if (int e = run_passes(sc, c, a, kn, ts.n, flags & RTW_FLAG_COUNT_TRAVERSAL, stream, &film)) return e;
    }
  }
  if (ev1) HIPCHK(hipEventRecord(ev1, stream), "hipEventRecord");
  return RTW_OK;
}

int enqueue_tonemap(const float* d_sum, uint32_t n_pixels, uint32_t spp, uint8_t* d_rgb8, hipStream_t stream) {
  if (!n_pixels) return RTW_OK;
  const float scale = 1.0f / (float)spp;  // rtw_tonemap's
  const uint32_t grid = (uint32_t)(((uint64_t)n_pixels + dev::FILM_BLOCK - 1u) / dev::FILM_BLOCK);
  hipLaunchKernelGGL(dev::tonemap_kernel, dim3(grid), dim3(dev::FILM_BLOCK), 0, stream, d_sum, n_pixels, scale, d_rgb8);
  HIPCHK(hipGetLastError(), "tonemap_kernel launch");
  return RTW_OK;
}

int enqueue_tile_noise(const float* d_sum, const float* d_sq, uint32_t w, uint32_t h, const uint32_t* d_ids_in,
                       uint32_t n_in, uint32_t samples, float threshold, float* d_err, uint32_t* d_tile_samples,
                       uint32_t* d_ids_out, uint32_t* d_n_out, hipStream_t stream) {
  const uint32_t tiles_x = (w + 7u) / 8u, n_tiles = tiles_x * ((h + 7u) / 8u);
  const float inv = 1.0f / (float)samples;  // one IEEE division, an argument of the kernel
  if (n_in) {
    const uint32_t per = dev::FILM_BLOCK / 64u;
    const uint32_t grid = (uint32_t)(((uint64_t)n_in + per - 1u) / per);
    hipLaunchKernelGGL(dev::tile_noise_kernel, dim3(grid), dim3(dev::FILM_BLOCK), 0, stream, d_sum, d_sq, w, h, tiles_x,
                       n_tiles, d_ids_in, n_in, samples, inv, threshold, d_err, d_tile_samples, d_ids_out);
    HIPCHK(hipGetLastError(), "tile_noise_kernel launch");
  }
  hipLaunchKernelGGL(dev::compact_tiles_kernel, dim3(1), dim3(dev::COMPACT_BLOCK), 0, stream, d_ids_in, n_in, d_ids_out,
                     d_n_out);
  HIPCHK(hipGetLastError(), "compact_tiles_kernel launch");
  return RTW_OK;
}

int enqueue_tonemap_tiles(const float* d_sum, uint32_t w, uint32_t h, const uint32_t* d_tile_samples, uint8_t* d_rgb8,
                          hipStream_t stream) {
  const uint64_t n = (uint64_t)w * h;
  const uint32_t grid = (uint32_t)((n + dev::FILM_BLOCK - 1u) / dev::FILM_BLOCK);
  hipLaunchKernelGGL(dev::tonemap_tiles_kernel, dim3(grid), dim3(dev::FILM_BLOCK), 0, stream, d_sum, w, h,
                     (w + 7u) / 8u, d_tile_samples, d_rgb8);
  HIPCHK(hipGetLastError(), "tonemap_tiles_kernel launch");
  return RTW_OK;
}

// The denoiser's launches: the prepare, `iterations` a-trous passes that ping-pong between the scratch's two record
// images (the last one writes d_out: the finish is fused into it), or prepare and finish alone for iterations = 0.
// Scratch layout, DENOISE_SCRATCH_PER_PIXEL = 64 bytes per pixel: X, Y, G, D images of one float4 each.
// Which steps take their taps through LDS: DENOISE_LDS_STEPS, bit k = the iteration of step 1 << k, measured on an
// MI355X at 1920x1080 (Denoiser); steps from 4 up read global memory.  Tuning knob
// RTW_DENOISE_LDS (a mask of bits 0-2) for the A/B.
constexpr uint32_t DENOISE_LDS_STEPS = 0x3u;
int enqueue_denoise(const float* d_sum, const float* d_sq, const float* d_albedo, const float* d_normal,
                    const float* d_depth, const float* d_count, uint32_t w, uint32_t h, uint32_t samples,
                    const uint32_t* d_tile_samples, uint32_t iterations, float sigma_l, float sigma_n, float sigma_z,
                    float* d_out, void* d_scratch, hipStream_t stream) {
  using namespace dev;
  const char* e = tuning_env("RTW_DENOISE_LDS");
  const uint32_t lds_steps = e ? ((uint32_t)atoi(e) & 0x7u) : DENOISE_LDS_STEPS;
  const size_t px = (size_t)w * h;
  float4* base = static_cast<float4*>(d_scratch);
  DenoiseArgs a;
  memset(&a, 0, sizeof a);
  a.sum = d_sum; a.sq = d_sq; a.albedo = d_albedo; a.normal = d_normal; a.depth = d_depth;
  a.tile_samples = d_tile_samples;
  a.count = d_count;
  a.w = w; a.h = h; a.tiles_x = (w + 7u) / 8u; a.samples = samples;
  a.X = base; a.Y = base + px; a.G = base + 2 * px; a.D = base + 3 * px;
  a.out = d_out;
  a.k_n = sigma_n != 0.0f ? 1.0f / (sigma_n * sigma_n) : 0.0f;
  a.sigma_l = sigma_l;
  a.use_n = sigma_n != 0.0f; a.use_z = sigma_z != 0.0f; a.use_l = sigma_l != 0.0f && d_sq != nullptr;
  const dim3 grid((w + DENOISE_TX - 1u) / DENOISE_TX, (h + DENOISE_TY - 1u) / DENOISE_TY), block(DENOISE_BLOCK);
  hipLaunchKernelGGL(denoise_prepare_kernel, grid, block, 0, stream, a);
  HIPCHK(hipGetLastError(), "denoise_prepare_kernel launch");
  if (iterations == 0) {
    hipLaunchKernelGGL(denoise_finish_kernel, grid, block, 0, stream, a);
    HIPCHK(hipGetLastError(), "denoise_finish_kernel launch");
    return RTW_OK;
  }
  for (uint32_t k = 0; k < iterations; ++k) {
    a.step = 1u << k;
    a.sz_step = sigma_z * (float)a.step;
    const bool lds = k < 3u && (lds_steps >> k & 1u), fin = k + 1u == iterations;
    const uint32_t lw = DENOISE_TX + 4u * a.step, lh = DENOISE_TY + 4u * a.step;
    const size_t lds_bytes = lds ? (size_t)lw * lh * 2u * sizeof(float4) : 0;
    if (lds && fin) hipLaunchKernelGGL((denoise_atrous_kernel<true, true>), grid, block, lds_bytes, stream, a);
    else if (lds) hipLaunchKernelGGL((denoise_atrous_kernel<true, false>), grid, block, lds_bytes, stream, a);
    else if (fin) hipLaunchKernelGGL((denoise_atrous_kernel<false, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((denoise_atrous_kernel<false, false>), grid, block, 0, stream, a);
    HIPCHK(hipGetLastError(), "denoise_atrous_kernel launch");
    std::swap(a.X, a.Y);
  }
  return RTW_OK;
}

// Temporal accumulation's launch: one thread per pixel, 32 x 8 pixels per workgroup as the denoiser's.
int enqueue_temporal(const TemporalArgs& a, hipStream_t stream) {
  using namespace dev;
  const dim3 grid((a.w + TEMPORAL_TX - 1u) / TEMPORAL_TX, (a.h + TEMPORAL_TY - 1u) / TEMPORAL_TY), block(TEMPORAL_BLOCK);
  hipLaunchKernelGGL(temporal_kernel, grid, block, 0, stream, a);
  HIPCHK(hipGetLastError(), "temporal_kernel launch");
  return RTW_OK;
}

// Ray queries (rtw_hit_rays*): the scene's variant as its renders pick it, the query kernel's own resident capacity
// as the largest grid, and the walk's launch tuning (leaf16, the spill split) as a render's.
int enqueue_hit_rays(Scene& sc, DeviceCopy& c, uint64_t n, const void* d_rays, void* d_hits, hipStream_t stream,
                     hipEvent_t ev0, hipEvent_t ev1) {
  const Knobs kn = read_knobs();
  const Variant var = path_kernel_variant(sc.flat, kn);
  const KernelCfg& k = var.cfg;
  const int resident = resident_blocks(c, GRID_HIT, (const void*)var.hit, k.blk, "query kernel", kn.verbose);
  const WalkTuning t = tune_walk(kn, sc.flat, k, resident);
  if (int e = grow(c.spill, (size_t)t.spill_depth * t.spill_lanes * sizeof(int32_t))) return e;
  QueryArgs a;
  memset(&a, 0, sizeof a);
  a.scene = c.scene;
  a.rays = d_rays;
  a.hits = d_hits;
  a.n = n;
  a.time_lo = sc.flat.time_lo;
  a.time_hi = sc.flat.time_hi;
  a.leaf16 = t.leaf16;
  a.spill_lanes = t.spill_lanes;
  a.spill = static_cast<int32_t*>(c.spill.p);
  a.err = c.err_host;
  return launch_query(var.hit, "hit_kernel launch", resident, k.blk, n, a, stream, ev0, ev1);
}

// Occlusion queries (rtw_occluded_rays*): enqueue_hit_rays' launch for the variant's occluded_kernel
int enqueue_occluded_rays(Scene& sc, DeviceCopy& c, uint64_t n, const void* d_rays, const float* d_t_max,
                          uint8_t* d_occluded, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  const Knobs kn = read_knobs();
  const Variant var = path_kernel_variant(sc.flat, kn);
  const KernelCfg& k = var.cfg;
  const int resident = resident_blocks(c, GRID_OCCLUDED, (const void*)var.occluded, k.blk, "occlusion kernel",
                                       kn.verbose);
  const WalkTuning t = tune_walk(kn, sc.flat, k, resident);
  if (int e = grow(c.spill, (size_t)t.spill_depth * t.spill_lanes * sizeof(int32_t))) return e;
  OccludedArgs a;
  memset(&a, 0, sizeof a);
  a.scene = c.scene;
  a.rays = d_rays;
  a.t_max = d_t_max;
  a.occluded = d_occluded;
  a.n = n;
  a.time_lo = sc.flat.time_lo;
  a.time_hi = sc.flat.time_hi;
  a.leaf16 = t.leaf16;
  a.spill_lanes = t.spill_lanes;
  a.spill = static_cast<int32_t*>(c.spill.p);
  a.err = c.err_host;
  return launch_query(var.occluded, "occluded_kernel launch", resident, k.blk, n, a, stream, ev0, ev1);
}

// Radiance queries (rtw_sample_rays*): the scene's variant and a render's whole launch tuning (tune_launch: quota16,
// leaf16, regen_min, the batch, the spill split) on the sample kernel's own resident capacity; the batch shrinks for a
// small launch by the render's rule (pass_batch; knob RTW_BATCH sets it outright).  The device copy's counters and
// dispenser words are zeroed on the stream first, and the dispenser again before every further launch of a long array.
int enqueue_sample_rays(Scene& sc, DeviceCopy& c, uint64_t n, const void* d_rays, const float* bg, uint32_t max_depth,
                        void* d_samples, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  const Knobs kn = read_knobs();
  const Variant var = path_kernel_variant(sc.flat, kn);
  const KernelCfg& k = var.cfg;
  const int resident = resident_blocks(c, GRID_SAMPLE, (const void*)var.sample, k.blk, "sample kernel", kn.verbose);
  const LaunchTuning t = tune_launch(kn, sc.flat, k, resident);
  if (int e = grow(c.spill, (size_t)t.walk.spill_depth * t.walk.spill_lanes * sizeof(int32_t))) return e;
  SampleArgs a;
  memset(&a, 0, sizeof a);
  a.scene = c.scene;
  a.max_depth = max_depth;
  memcpy(a.bg, bg, sizeof a.bg);
  a.time_lo = sc.flat.time_lo;
  a.time_hi = sc.flat.time_hi;
  a.quota16 = t.quota16;
  a.leaf16 = t.walk.leaf16;
  a.regen_min = t.regen_min;
  a.spill_lanes = t.walk.spill_lanes;
  a.spill = static_cast<int32_t*>(c.spill.p);
  a.counters = c.counters;
  a.queue = dispensers(c);
  a.err = c.err_host;
  const uint64_t waves = (uint64_t)resident * (uint32_t)k.blk / 64u;
  HIPCHK(hipMemsetAsync(c.counters, 0, COUNTER_WORDS * sizeof(unsigned long long), stream), "hipMemsetAsync");
  if (ev0) HIPCHK(hipEventRecord(ev0, stream), "hipEventRecord");
  for (uint64_t first = 0; first < n; first += SAMPLE_LAUNCH_MAX) {
    const uint64_t m = std::min(SAMPLE_LAUNCH_MAX, n - first);
    if (first) HIPCHK(hipMemsetAsync(a.queue, 0, DISP * DISP_STRIDE * sizeof(unsigned long long), stream),
                      "hipMemsetAsync(queue)");
    a.rays = static_cast<const char*>(d_rays) + first * sizeof(rtw_ray);
    a.samples = static_cast<char*>(d_samples) + first * sizeof(rtw_sample);
    a.n = (uint32_t)m;
    a.batch = kn.batch.set ? t.batch : pass_batch(t.batch, m, waves);
    // persistent: at most the resident capacity, and no more workgroups than the rays can occupy
    const int grid = (int)std::min<uint64_t>((uint64_t)resident, (m + (uint32_t)k.blk - 1u) / (uint32_t)k.blk);
    hipLaunchKernelGGL(var.sample, dim3(grid), dim3(k.blk), 0, stream, a);
    HIPCHK(hipGetLastError(), "sample_kernel launch");
  }
  if (ev1) HIPCHK(hipEventRecord(ev1, stream), "hipEventRecord");
  return RTW_OK;
}

// Scatter queries (rtw_scatter_rays*): the scene's tables, the per-material shading records and the record arrays.
int enqueue_scatter_rays(Scene& sc, DeviceCopy& c, uint64_t n, const void* d_rays, const void* d_hits, const float* bg,
                         void* d_out_rays, void* d_out_scatter, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  const Knobs kn = read_knobs();
  ScatterArgs a;
  memset(&a, 0, sizeof a);
  a.scene = c.scene;
  a.mshade = static_cast<const DevShade*>(c.mshade.p);
  a.n_mats = (uint32_t)sc.flat.mshade.size();
  memcpy(a.bg, bg, sizeof a.bg);
  a.rays = d_rays;
  a.hits = d_hits;
  a.out_rays = d_out_rays;
  a.out_scatter = d_out_scatter;
  a.n = n;
  const int resident = resident_blocks(c, GRID_SCATTER, (const void*)dev::scatter_kernel, dev::SHADE_BLOCK,
                                       "scatter_kernel", kn.verbose);
  return launch_query(dev::scatter_kernel, "scatter_kernel launch", resident, dev::SHADE_BLOCK, n, a, stream, ev0, ev1);
}

// Camera-ray queries (rtw_camera_rays*): start_path's operands as frame_args computes them for a render of the frame.
int enqueue_camera_rays(DeviceCopy& c, const Frame& f, uint64_t first, uint64_t n, void* d_rays, hipStream_t stream,
                        hipEvent_t ev0, hipEvent_t ev1) {
  const Knobs kn = read_knobs();
  const RenderArgs r = frame_args(c, f, TileSet{}, nullptr);
  CameraRaysArgs a;
  memset(&a, 0, sizeof a);
  a.cam = r.cam;
  a.fw1 = r.fw1; a.fh1 = r.fh1; a.rw1 = r.rw1; a.rh1 = r.rh1; a.time_span = r.time_span;
  a.w = f.w; a.spp = f.spp;
  a.row_paths = (uint64_t)f.w * f.spp;
  a.h1 = f.h - 1u;
  a.seed_hash = r.seed_hash;
  a.first = first;
  a.n = n;
  a.rays = d_rays;
  const int resident = resident_blocks(c, GRID_CAMERA, (const void*)dev::camera_rays_kernel, dev::SHADE_BLOCK,
                                       "camera_rays_kernel", kn.verbose);
  return launch_query(dev::camera_rays_kernel, "camera_rays_kernel launch", resident, dev::SHADE_BLOCK, n, a, stream,
                      ev0, ev1);
}

// Feature buffers (rtw_render_features*): the scene's variant as its renders pick it, the feature kernel's own resident
// capacity as the largest grid (one wave per tile slot), the walk's launch tuning as a render's, frame_args' camera
// operands.  The counters are zeroed on the stream first: the kernel adds the samples it traced to the first word.
int enqueue_features(Scene& sc, DeviceCopy& c, const Frame& f, uint32_t sample_first, const TileSet& ts,
                     float* d_albedo, float* d_normal, float* d_depth, hipStream_t stream, hipEvent_t ev0,
                     hipEvent_t ev1) {
  if (int e = check_guard(c)) return e;
  if (int e = check_image_max(f.w, f.h)) return e;
  if (int e = check_shutter(*f.cam, sc.flat)) return e;
  const Knobs kn = read_knobs();
  const Variant var = path_kernel_variant(sc.flat, kn);
  const KernelCfg& k = var.cfg;
  const int resident = resident_blocks(c, GRID_FEATURE, (const void*)var.feature, k.blk, "feature kernel", kn.verbose);
  const WalkTuning t = tune_walk(kn, sc.flat, k, resident);
  if (int e = grow(c.spill, (size_t)t.spill_depth * t.spill_lanes * sizeof(int32_t))) return e;
  Frame f0 = f;
  f0.sample_base = 0;  // the key's sample word is the kernel's own s
  const RenderArgs r = frame_args(c, f0, ts, nullptr);
  FeatureArgs a;
  memset(&a, 0, sizeof a);
  a.scene = c.scene;
  a.mshade = static_cast<const DevShade*>(c.mshade.p);
  a.cam = r.cam;
  memcpy(a.bg, f.bg, sizeof a.bg);
  a.fw1 = r.fw1; a.fh1 = r.fh1; a.rw1 = r.rw1; a.rh1 = r.rh1; a.time_span = r.time_span;
  a.w = f.w; a.h = f.h; a.tiles_x = r.tiles_x;
  a.n_tiles = (uint32_t)f.tiles();
  a.seed_hash = r.seed_hash;
  a.sample_first = sample_first;
  a.n_samples = f.spp;
  a.tile_ids = ts.ids;
  a.n_slots = ts.n;
  a.packed = r.packed_out;
  a.albedo = d_albedo;
  a.normal = d_normal;
  a.depth = d_depth;
  a.leaf16 = t.leaf16;
  a.spill_lanes = t.spill_lanes;
  a.spill = static_cast<int32_t*>(c.spill.p);
  a.err = c.err_host;
  a.counters = c.counters;
  HIPCHK(hipMemsetAsync(c.counters, 0, COUNTER_WORDS * sizeof(unsigned long long), stream), "hipMemsetAsync");
  // one wave per tile slot
  return launch_query(var.feature, "feature_kernel launch", resident, k.blk, (uint64_t)ts.n * 64u, a, stream, ev0, ev1);
}

// Ambient occlusion (rtw_render_ao*): enqueue_features' launch for the variant's ao_kernel.  The kernel adds the camera
// samples it traced to the counters' first word and the AO rays it cast to the second.
int enqueue_ao(Scene& sc, DeviceCopy& c, const Frame& f, uint32_t sample_first, const TileSet& ts, uint32_t ao_rays,
               float radius, float* d_ao, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  if (int e = check_guard(c)) return e;
  if (int e = check_image_max(f.w, f.h)) return e;
  if (int e = check_shutter(*f.cam, sc.flat)) return e;
  const Knobs kn = read_knobs();
  const Variant var = path_kernel_variant(sc.flat, kn);
  const KernelCfg& k = var.cfg;
  const int resident = resident_blocks(c, GRID_AO, (const void*)var.ao, k.blk, "ao kernel", kn.verbose);
  const WalkTuning t = tune_walk(kn, sc.flat, k, resident);
  if (int e = grow(c.spill, (size_t)t.spill_depth * t.spill_lanes * sizeof(int32_t))) return e;
  Frame f0 = f;
  f0.sample_base = 0;  // the key's sample word is the kernel's own s
  const RenderArgs r = frame_args(c, f0, ts, nullptr);
  AoArgs a;
  memset(&a, 0, sizeof a);
  a.scene = c.scene;
  a.cam = r.cam;
  a.fw1 = r.fw1; a.fh1 = r.fh1; a.rw1 = r.rw1; a.rh1 = r.rh1; a.time_span = r.time_span;
  a.w = f.w; a.h = f.h; a.tiles_x = r.tiles_x;
  a.n_tiles = (uint32_t)f.tiles();
  a.seed_hash = r.seed_hash;
  a.sample_first = sample_first;
  a.n_samples = f.spp;
  a.ao_rays = ao_rays;
  a.radius = radius;
  a.tile_ids = ts.ids;
  a.n_slots = ts.n;
  a.packed = r.packed_out;
  a.ao = d_ao;
  a.leaf16 = t.leaf16;
  a.spill_lanes = t.spill_lanes;
  a.spill = static_cast<int32_t*>(c.spill.p);
  a.err = c.err_host;
  a.counters = c.counters;
  HIPCHK(hipMemsetAsync(c.counters, 0, COUNTER_WORDS * sizeof(unsigned long long), stream), "hipMemsetAsync");
  // one wave per tile slot
  return launch_query(var.ao, "ao_kernel launch", resident, k.blk, (uint64_t)ts.n * 64u, a, stream, ev0, ev1);
}

int enqueue_unpack(uint32_t w, uint32_t h, const uint32_t* d_tiles, uint32_t n_tiles, const float* d_packed,
                   float* d_image, hipStream_t stream) {
  const uint32_t n = n_tiles * 64u;
  if (!n) return RTW_OK;
  hipLaunchKernelGGL(dev::unpack_tiles_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, w, h, (w + 7u) / 8u, d_tiles,
                     n_tiles, d_packed, d_image);
  HIPCHK(hipGetLastError(), "unpack_tiles_kernel");
  return RTW_OK;
}

// a diagnostic call's device array of n Ts, freed on every return path
template <class T>
struct DiagBuf {
  T* p = nullptr;
  bool alloc(size_t n) { return hipMalloc((void**)&p, n * sizeof(T)) == hipSuccess; }
  ~DiagBuf() { hipFree(p); }
};

}  // namespace rtw

using namespace rtw;

extern "C" {

int rtw_diag_libm(int fn, uint32_t n, const float* a, const float* b, float* out) {
  if (fn < 0 || fn > 5 || (n && (!a || !out || ((fn == 3 || fn == 4) && !b)))) return fail(RTW_EINVAL, "bad arguments");
  if (!n) return RTW_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(RTW_ENODEV, "no HIP device visible");
  DiagBuf<float> da, db, dout;
  const size_t bytes = (size_t)n * sizeof(float);
  if (!da.alloc(n) || !dout.alloc(n) || ((fn == 3 || fn == 4) && !db.alloc(n))) return fail(RTW_ENOMEM, "hipMalloc(diag)");
  if (hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice) != hipSuccess ||
      (db.p && hipMemcpy(db.p, b, bytes, hipMemcpyHostToDevice) != hipSuccess))
    return fail(RTW_ENODEV, "hipMemcpy(diag)");
  hipLaunchKernelGGL(dev::libm_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, fn, n, da.p, db.p, dout.p);
  if (hipGetLastError() != hipSuccess || hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(RTW_ENODEV, "libm_kernel");
  return RTW_OK;
}

int rtw_diag_tile_lists(rtw_scene* s, int device, const rtw_camera* cam, uint32_t w, uint32_t h, uint32_t* records,
                        uint64_t cap_words, uint32_t* n_over, uint32_t* prim_keys, uint32_t cap_keys) {
  if (!s || !cam || !records) return fail(RTW_EINVAL, "NULL argument");
  if (!s->s.committed) return fail(RTW_ESTATE, "scene not committed");
  if (int e = check_image_min(w, h)) return e;
  if (int e = check_image_max(w, h)) return e;
  DeviceCopy* c = need_copy(s->s, device);
  if (!c) return RTW_ENODEV;
  const uint32_t n_bvh = s->s.flat.far.n_bvh;
  if (!c->pboxes.p || n_bvh == 0 || n_bvh >= TILE_LIST_OVER || s->s.flat.pboxes.size() != (size_t)n_bvh * 8u)
    return fail(RTW_EINVAL, "the scene has no sphere BVH of under %u primitives: no tile lists", TILE_LIST_OVER);
  const uint64_t words = (uint64_t)((w + 7u) / 8u) * ((h + 7u) / 8u) * TILE_LIST_WORDS;
  if (cap_words < words) return fail(RTW_EINVAL, "records: %llu words needed", (unsigned long long)words);
  const Knobs kn = read_knobs();
  const uint32_t cap = (uint32_t)std::min((int)TILE_LIST_MAX, std::max(1, kn.tile_list_cap.get((int)TILE_LIST_MAX)));
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  DiagBuf<uint32_t> lists, over;
  if (!lists.alloc(words) || !over.alloc(1)) return fail(RTW_ENOMEM, "hipMalloc(tile lists)");
  if (int e = enqueue_tile_lists(s->s, *c, *cam, w, h, cap, lists.p, over.p, nullptr)) return e;
  uint32_t no = 0;
  if (hipMemcpy(records, lists.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&no, over.p, sizeof no, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(RTW_ENODEV, "tile_list_kernel");
  if (n_over) *n_over = no;
  for (uint32_t k = 0; prim_keys && k < std::min(cap_keys, n_bvh); ++k) prim_keys[k] = s->s.flat.prims[k].key;
  return (int)n_bvh;
}

int rtw_diag_tile_beam(const rtw_camera* cam, uint32_t w, uint32_t h, uint32_t tile, const float* box_lo,
                       const float* box_hi) {
  if (!cam || !box_lo || !box_hi) return fail(RTW_EINVAL, "NULL argument");
  if (int e = check_image_min(w, h)) return e;
  const BeamCamera C = beam_camera(cam->origin, cam->u, cam->v, cam->lower_left_corner, cam->horizontal, cam->vertical,
                                   cam->lens_radius);
  return beam_may_hit(C, beam_tile(C, w, h, tile), beam_box(C, box_lo, box_hi)) ? 1 : 0;
}

int rtw_diag_sweep(int fn, uint32_t lo, uint32_t hi, uint64_t* counts, uint32_t* bad, uint32_t cap) {
  if (fn != 0 || lo > hi || !counts || (cap && !bad)) return fail(RTW_EINVAL, "bad arguments");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(RTW_ENODEV, "no HIP device visible");
  DiagBuf<unsigned long long> dn;
  DiagBuf<uint32_t> dbad;
  if (!dn.alloc(3) || !dbad.alloc(cap ? cap : 1)) return fail(RTW_ENOMEM, "hipMalloc(sweep)");
  if (hipMemset(dn.p, 0, 3 * sizeof(unsigned long long)) != hipSuccess) return fail(RTW_ENODEV, "hipMemset(sweep)");
  hipLaunchKernelGGL(dev::sweep_kernel, dim3(16384), dim3(256), 0, nullptr, fn, lo, hi, dn.p, dbad.p, cap);
  unsigned long long h[3];
  if (hipGetLastError() != hipSuccess || hipMemcpy(h, dn.p, sizeof h, hipMemcpyDeviceToHost) != hipSuccess ||
      (cap && hipMemcpy(bad, dbad.p, cap * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess))
    return fail(RTW_ENODEV, "sweep_kernel");
  counts[0] = h[0];
  counts[1] = h[1];
  return RTW_OK;
}

}  // extern "C"
