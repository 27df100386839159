// rtw_shade_kernel.hpp — the second half of a caller's own integrator (rtw_camera_rays*, rtw_scatter_rays*): the
// render's camera and materials as batch queries over the committed scene's own tables.  camera_rays_kernel is
// start_path's ray (lib.rs:84-86, camera.rs:66-74) for path p of a frame; scatter_kernel is one step of sample_ray
// after world.hit (lib.rs:102-116): Material::scatter (material.rs:42-165) and Material::emitted (light_source.rs:17-24) for a hit
// record rtw_hit_rays produced, the background for a miss.  The same helpers, f32 operations and draw order as
// path_kernel, so camera_rays -> (hit_rays -> scatter_rays)* reproduces the render bit for bit.
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

// a ray record (40 B, on an 8-byte boundary) as two quads and the stream pair
__device__ __forceinline__ void store_ray(void* rays, uint64_t i, ray_quad q0, ray_quad q1, ray_pair q2) {
  char* rp = reinterpret_cast<char*>(rays) + i * sizeof(rtw_ray);
  *reinterpret_cast<ray_quad*>(rp) = q0;
  *reinterpret_cast<ray_quad*>(rp + 16) = q1;
  *reinterpret_cast<ray_pair*>(rp + 32) = q2;
}

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
    uint64_t rng = xoro_seed(splitmix64(a.seed_hash ^ (((uint64_t)j << 48) | ((uint64_t)i << 32) | s)));
    // lib.rs:84-86 + camera.rs:66-74
    const float u = div_by_recip((float)i + gen_f32(rng), a.fw1, a.rw1);
    const float v = div_by_recip((float)j + gen_f32(rng), a.fh1, a.rh1);
    const V3 rd = scale(rand_in_unit_disk<false>(rng), C.lens_radius);
    const V3 off = add(scale(ld3(C.u), rd.x), scale(ld3(C.v), rd.y));
    const V3 o = add(ld3(C.origin), off);
    const V3 d = sub(sub(add(add(ld3(C.llc), scale(ld3(C.horizontal), u)), scale(ld3(C.vertical), v)), ld3(C.origin)),
                     off);
    const float time = gen_range<false>(rng, C.time0, C.time1, a.time_span);
    ray_quad q0, q1;
    ray_pair q2;
    q0.x = o.x; q0.y = o.y; q0.z = o.z; q0.w = d.x;
    q1.x = d.y; q1.y = d.z; q1.z = time; q1.w = 0.0f;
    q2.x = (uint32_t)rng; q2.y = (uint32_t)(rng >> 32);
    store_ray(a.rays, k, q0, q1, q2);
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
    const char* rp = reinterpret_cast<const char*>(a.rays) + i * sizeof(rtw_ray);
    const ray_quad r0 = *reinterpret_cast<const ray_quad*>(rp);       // origin, direction.x
    const ray_quad r1 = *reinterpret_cast<const ray_quad*>(rp + 16);  // direction.y, .z, time, reserved
    const ray_pair r2 = *reinterpret_cast<const ray_pair*>(rp + 32);  // stream
    const float4* hp = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(a.hits) + i * sizeof(rtw_hit));
    const float4 h0 = hp[0], h1 = hp[1], h2 = hp[2];  // p, normal.x | normal.y, .z, t, u | v, material, key, flags
    const uint64_t word = ((uint64_t)r2.y << 32) | r2.x;
    // The caller supplies the generator state and the rejection loops below are unbounded: xoroshiro64* never leaves
    // state 0, so the state is mended here, before anything can draw from it (a zero word is marked BAD besides).
    uint64_t rng = xoro_seed(word);
    const V3 d_in = mk(r0.w, r1.x, r1.y);
    const uint32_t mat = __float_as_uint(h2.y), hflags = __float_as_uint(h2.w);
    const bool is_hit = (hflags & (uint32_t)RTW_HIT_HIT) != 0u;
    // (the material id is checked before any table is read with it)
    const bool bad = word == 0ull || (hflags & (uint32_t)RTW_HIT_BAD_RAY) != 0u || (is_hit && mat >= a.n_mats);
    ray_quad q0 = r0, q1 = r1;  // a miss: the ray copied through
    ray_pair q2 = r2;
    V3 att = mk(0.f, 0.f, 0.f), emit = ld3(a.bg);  // lib.rs:102-105
    uint32_t flags = (uint32_t)RTW_SCATTER_MISS;
    if (bad) {
      q0.x = q0.y = q0.z = q0.w = 0.0f;
      q1 = q0;
      q2.x = q2.y = 0u;
      emit = att;
      flags = (uint32_t)RTW_SCATTER_BAD;
    } else if (is_hit) {
      const V3 hp3 = mk(h0.x, h0.y, h0.z), hn = mk(h0.w, h1.x, h1.y);
      const float hu = h1.w, hv = h2.x;
      const bool front = (hflags & (uint32_t)RTW_HIT_FRONT_FACE) != 0u;
      const DevShade sh = a.mshade[mat];
      // One body for every material (material.rs:42-165, light_source.rs:17-24), as path_kernel's: a wave mixing
      // materials runs the rejection loop, unit() and the texture lookup once.
      const uint32_t mt = sh.kind & 0xffu, mode = (sh.kind >> 8) & 0xfu;
      const bool light = mt == MT_LIGHT, lam = mt == MT_LAMBERT, met = mt == MT_METAL, iso = mt == MT_ISOTROPIC;
      V3 rs = mk(0.f, 0.f, 0.f);
      if (lam || met || iso) rs = rand_in_unit_sphere<false>(rng);  // vec3.rs:101-108
      const V3 ud = unit(lam ? rs : d_in);                           // Lambertian: unit(rs); else unit(d_in)
      V3 tv = mk(1.f, 1.f, 1.f);                                     // Dielectric: attenuation (1,1,1)
      if (met) {
        tv = ld3(sh.a);
      } else if (light || lam || iso) {
        if (mode == SM_SOLID) tv = ld3(sh.a);  // SolidColor::value
        else if (mode == SM_CHECKER)
          tv = checker_odd(sh.param * hp3.x, sh.param * hp3.y, sh.param * hp3.z) ? ld3(sh.a) : ld3(sh.b);
        else if (mode == SM_IMAGE)
          tv = image_texel(S, __float_as_uint(sh.a[0]), __float_as_uint(sh.a[1]), __float_as_uint(sh.a[2]), hu, hv);
        else tv = tex_value<F_ALL>(S, S.mats[mat].tex, hu, hv, hp3);
      }
      bool scattered = false;
      V3 dir = d_in;  // (a light: the incoming direction, not a ray to follow)
      emit = mk(0.f, 0.f, 0.f);
      if (light) {  // emit, no scatter, no draws
        emit = tv;
      } else {
        scattered = true;
        dir = rs;   // Isotropic (material.rs:155-165): never absorbs
        if (lam) {  // material.rs:42-56
          dir = add(hn, ud);
          if (near_zero(dir)) dir = hn;
        } else if (met) {  // material.rs:78-95
          dir = add(reflect(ud, hn), scale(rs, sh.param));
          scattered = dot(dir, hn) > 0.0f;  // else absorbed: emitted() is black
        } else if (!iso) {  // Dielectric, material.rs:116-142; 1 / ir and both r0: the flattener's bits (DevShade::a)
          const float ratio = front ? sh.a[0] : sh.param;
          const float r0s = front ? sh.a[1] : sh.a[2];
          const float cos_t = fminf(dot(neg(ud), hn), 1.0f);
          const float sin_t = sqrtf(1.0f - cos_t * cos_t);
          const bool cannot = (ratio * sin_t) > 1.0f;
          if (cannot || reflectance(cos_t, r0s) > gen_f32(rng)) dir = reflect(ud, hn);
          else dir = refract(ud, hn, ratio);
        }
        if (scattered) att = tv;
      }
      q0.x = hp3.x; q0.y = hp3.y; q0.z = hp3.z; q0.w = dir.x;
      q1.x = dir.y; q1.y = dir.z;  // time and reserved kept
      q2.x = (uint32_t)rng; q2.y = (uint32_t)(rng >> 32);
      flags = scattered ? (uint32_t)RTW_SCATTER_SCATTERED : 0u;
    }
    store_ray(a.out_rays, i, q0, q1, q2);
    float4* sp = reinterpret_cast<float4*>(reinterpret_cast<char*>(a.out_scatter) + i * sizeof(rtw_scatter));
    sp[0] = make_float4(att.x, att.y, att.z, emit.x);
    sp[1] = make_float4(emit.y, emit.z, __uint_as_float(flags), __uint_as_float(0u));
  }
}

}  // namespace dev
}  // namespace rtw
