// rtw_shade_kernel.hpp — the second half of a caller's own integrator (rtw_camera_rays*, rtw_scatter_rays*): the
// render's camera and materials as batch queries over the committed scene's own tables.  camera_rays_kernel is
// start_path's ray (lib.rs:84-86, camera.rs:66-74) for path p of a frame; scatter_kernel is one step of sample_ray
// after world.hit (lib.rs:102-116): Material::scatter (material.rs:42-165) and Material::emitted (light_source.rs:17-24) for a hit
// record rtw_hit_rays produced, the background for a miss.  scatter_kernel shades with the materials' one body
// (rtw_dev_shade.hpp), which path_kernel calls too; camera_rays_kernel restates start_path's f32 operations and draw
// order.  So camera_rays -> (hit_rays -> scatter_rays)* reproduces the render bit for bit.
//
// One instantiation each, with every texture kind (F_ALL): these kernels stream records and are not register-bound.
// Both read immutable scene tables only -- no spill area, path queue or sample buffer -- so they need not be serialised
// with the scene's renders.  Included by rtw_kernel.hip alone.
#pragma once
#include "../../include/rtw.h"
#include "rtw_query_kernel.hpp"

namespace rtw {

struct CameraRaysArgs {
  DevCamera cam;
  float fw1, fh1, rw1, rh1, time_span;  // RenderArgs' (frame_args computes both from the same frame)
  uint32_t w, spp;
  uint64_t row_paths;  // w * spp: paths per image row
  uint32_t h1;         // h - 1
  uint64_t seed_hash;  // splitmix64(seed)
  uint64_t first, n;   // ray k is path first + k of the frame, in rtw_render's output order
  void* rays;          // rtw_ray[n], 16-byte aligned
};

struct ScatterArgs {
  DevScene scene;
  const DevShade* mshade;  // one shading record per material (Flat::mshade)
  uint32_t n_mats;
  float bg[3];
  const void* rays;   // rtw_ray[n]
  const void* hits;   // rtw_hit[n]
  void* out_rays;     // rtw_ray[n]; may be `rays`
  void* out_scatter;  // rtw_scatter[n]
  uint64_t n;
};

namespace dev {

static_assert(sizeof(rtw_scatter) == 32, "rtw_scatter layout (include/rtw.h)");
constexpr int SHADE_BLOCK = 256;

// start_path (rtw_path_kernel.hpp, AB = false) for the pixel and sample decoded from the path's place in the output:
// p = (row * w + i) * spp + s, row = h - 1 - j.  The stream word is the generator's state after the time draw.
__global__ __launch_bounds__(SHADE_BLOCK) void camera_rays_kernel(CameraRaysArgs a) {
  const DevCamera& C = a.cam;
  const uint64_t stride = (uint64_t)gridDim.x * SHADE_BLOCK;
  for (uint64_t k = (uint64_t)blockIdx.x * SHADE_BLOCK + threadIdx.x; k < a.n; k += stride) {
    const uint64_t p = a.first + k;
    const uint64_t row = p / a.row_paths, in_row = p - row * a.row_paths;
    const uint32_t i = (uint32_t)(in_row / a.spp), s = (uint32_t)(in_row - (uint64_t)i * a.spp);
    const uint32_t j = a.h1 - (uint32_t)row;
    Ray r;
    const uint64_t rng = camera_ray(C, a.fw1, a.fh1, a.rw1, a.rh1, a.time_span, a.seed_hash, j, i, s, r);
    const V3 o = r.o, d = r.d;
    const float time = r.time;
    RayRec q;
    q.q0.x = o.x; q.q0.y = o.y; q.q0.z = o.z; q.q0.w = d.x;
    q.q1.x = d.y; q.q1.y = d.z; q.q1.z = time; q.q1.w = 0.0f;
    q.q2.x = (uint32_t)rng; q.q2.y = (uint32_t)(rng >> 32);
    store_ray(a.rays, k, q);
  }
}

// One record per lane, grid-stride.  A lane reads its ray and its hit record whole before it writes, so out_rays may be
// the input array.  waves_per_eu(5, 8): left alone the allocator takes 97 VGPRs, one over the 5-wave bound; asked for 5
// waves it takes 81, still without scratch (MI355X, jumpy-balls' / the cow's primary hits: 27.0 / 29.3 G records/s in
// the 4-wave build's one run, 27.6 / 30.7 and 29.0 / 31.2 in the 5-wave build's two: a gain the size of the spread).
__global__ __launch_bounds__(SHADE_BLOCK) __attribute__((amdgpu_waves_per_eu(5, 8))) void scatter_kernel(
    ScatterArgs a) {
  const DevScene& S = a.scene;
  const uint64_t stride = (uint64_t)gridDim.x * SHADE_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * SHADE_BLOCK + threadIdx.x; i < a.n; i += stride) {
    const RayRec r = load_ray(a.rays, i);
    const float4* hp = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(a.hits) + i * sizeof(rtw_hit));
    const float4 h0 = hp[0], h1 = hp[1], h2 = hp[2];  // p, normal.x | normal.y, .z, t, u | v, material, key, flags
    Ray ray;  // (its direction: the rest of a scatter is the hit record's)
    const uint64_t word = ray_of(r, ray);
    // The caller supplies the generator state and the rejection loops below are unbounded: xoroshiro64* never leaves
    // state 0, so the state is mended here, before anything can draw from it (a zero word is marked BAD besides).
    uint64_t rng = xoro_seed(word);
    const uint32_t mat = __float_as_uint(h2.y), hflags = __float_as_uint(h2.w);
    const bool is_hit = (hflags & (uint32_t)RTW_HIT_HIT) != 0u;
    // (the material id is checked before any table is read with it)
    const bool bad = word == 0ull || (hflags & (uint32_t)RTW_HIT_BAD_RAY) != 0u || (is_hit && mat >= a.n_mats);
    RayRec q = r;  // a miss: the ray copied through
    V3 att = mk(0.f, 0.f, 0.f), emit = ld3(a.bg);  // lib.rs:102-105
    uint32_t flags = (uint32_t)RTW_SCATTER_MISS;
    if (bad) {
      q.q0.x = q.q0.y = q.q0.z = q.q0.w = 0.0f;
      q.q1 = q.q0;
      q.q2.x = q.q2.y = 0u;
      emit = att;
      flags = (uint32_t)RTW_SCATTER_BAD;
    } else if (is_hit) {
      Rec h;
      h.p = mk(h0.x, h0.y, h0.z);
      h.n = mk(h0.w, h1.x, h1.y);
      h.u = h1.w;
      h.v = h2.x;
      h.front = (hflags & (uint32_t)RTW_HIT_FRONT_FACE) != 0u;
      h.mat = mat;
      const DevShade sh = a.mshade[mat];
      // the materials' one body (rtw_dev_shade.hpp), the rejection draw and unit() between its pieces
      const MatKind kind = mat_kind<F_ALL>(sh.kind);
      V3 rs = mk(0.f, 0.f, 0.f);
      if (kind.lam || kind.met || kind.iso) rs = rand_in_unit_sphere<false>(rng);  // vec3.rs:101-108
      const V3 ud = unit(kind.lam ? rs : ray.d);  // Lambertian: unit(rs); else unit(d_in)
      const V3 tv = mat_attenuation<F_ALL>(S, sh, kind, h, [&] { return ld3(sh.b); });
      bool absorbed = false;
      V3 dir = ray.d;  // (a light: the incoming direction, not a ray to follow)
      emit = mk(0.f, 0.f, 0.f);
      if (kind.light) {  // emit, no scatter, no draws
        emit = tv;
      } else {
        dir = mat_direction<F_ALL>(sh, kind, h, ud, rs, rng, absorbed);
        if (!absorbed) att = tv;
      }
      const bool scattered = !kind.light && !absorbed;
      q.q0.x = h.p.x; q.q0.y = h.p.y; q.q0.z = h.p.z; q.q0.w = dir.x;
      q.q1.x = dir.y; q.q1.y = dir.z;  // time and reserved kept
      q.q2.x = (uint32_t)rng; q.q2.y = (uint32_t)(rng >> 32);
      flags = scattered ? (uint32_t)RTW_SCATTER_SCATTERED : 0u;
    }
    store_ray(a.out_rays, i, q);
    float4* sp = reinterpret_cast<float4*>(reinterpret_cast<char*>(a.out_scatter) + i * sizeof(rtw_scatter));
    sp[0] = make_float4(att.x, att.y, att.z, emit.x);
    sp[1] = make_float4(emit.y, emit.z, __uint_as_float(flags), __uint_as_float(0u));
  }
}

}  // namespace dev
}  // namespace rtw
