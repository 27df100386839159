// rtw_dev_shade.hpp — what shading needs of the winner: its hit record (Rec, hit_record: hittable/mod.rs:32-48), the
// textures (checker, Perlin noise, image lookup, tex_value: texture.rs, image_texture.rs, perlin.rs) and Schlick's
// reflectance, and the materials (mat_kind, mat_attenuation, mat_direction): the one body that path_kernel,
// sample_kernel and scatter_kernel all shade with.
#pragma once
#include "rtw_dev_hit.hpp"

#include "rtw_checker.h"  // (after the HIP runtime: its functions are __host__ __device__)

namespace rtw {
namespace dev {

// ---- hit record of the winner (hittable/mod.rs:32-48 at every level)
struct Rec { V3 p, n; float u, v; bool front; uint32_t mat; };
__device__ __forceinline__ void face(Rec& h, V3 dir, V3 outward) {
  h.front = dot(dir, outward) < 0.0f;
  h.n = h.front ? outward : neg(outward);
}
__device__ __forceinline__ void sphere_uv(V3 p, float& u, float& v) {  // spherical.rs:62-77
  const float PI = 3.14159265358979323846f;
  float theta = dev_acosf(-p.y);
  float phi = dev_atan2f(-p.z, p.x) + PI;
  u = phi / (2.0f * PI);
  v = theta / PI;
}

template <uint32_t FEAT>
__device__ Rec hit_record(const DevScene& S, const Ray& wr, const Best& b, uint32_t shade_kind) {
  // Triangle kernels: the meta word first, then only the geometry the winner's type needs (a triangle
  // needs none: its barycentrics come from its test, Best::u / v; cow +4%).  Other kernels load the whole
  // record in one round trip (a dependent geometry load cost jumpy 2.3%, profiles/r03/experiments b2).
  const float4* PP = reinterpret_cast<const float4*>(S.prims + b.prim);
  const uint4 meta = *reinterpret_cast<const uint4*>(PP + 3);
  float4 g0, g1, g2;
  if constexpr (!(FEAT & F_TRI)) {
    g0 = PP[0];
    g1 = PP[1];
    g2 = PP[2];
  }
  auto geo = [&](int k) -> float4 {
    if constexpr (!(FEAT & F_TRI)) return k == 0 ? g0 : (k == 1 ? g1 : g2);
    else return PP[k];
  };
  const uint32_t type = meta.x & 0xffu, inst = meta.x >> 8;
  const DevInst* I = S.insts + inst;
  const bool uni = (FEAT & F_INST) && inst && inst == S.uni_inst;  // one Translation, offset uniform
  Ray lr = wr;
  // Chains of at most two wrappers (a Cuboid's .rotate_y().translate(): cornell-box, the book-2 scenes), in the
  // kernels without triangles: the header and both ops in three independent loads and the directions after each op
  // kept for the unwinding below, instead of the generic loops' chain of dependent loads and per-level recomputation
  // (the same f32 operations).
  bool short_chain = false;
  uint32_t nops = 0;
  float4 op0 = make_float4(0.f, 0.f, 0.f, 0.f), op1 = op0;
  V3 d0 = wr.d, d1 = wr.d;  // the ray direction inside wrapper 0 (after op 0) and wrapper 1 (after ops 0, 1)
  auto apply_op = [](float4 op, Ray& r) {  // transformations.rs:23-28 / :115-135, as to_local
    if (op_is(op.x, IO_TRANSLATE)) {
      r.o = sub(r.o, mk(op.y, op.z, op.w));
    } else {
      const float s = op.y, c = op.z;
      r.o = mk(c * r.o.x - s * r.o.z, r.o.y, s * r.o.x + c * r.o.z);
      r.d = mk(c * r.d.x - s * r.d.z, r.d.y, s * r.d.x + c * r.d.z);
    }
  };
  if (uni) {
    lr.o = sub(wr.o, mk(S.uni_off[0], S.uni_off[1], S.uni_off[2]));
  } else if ((FEAT & F_INST) && inst) {
    nops = I->nops;
    op0 = *reinterpret_cast<const float4*>(I->op[0]);
    op1 = *reinterpret_cast<const float4*>(I->op[1]);
    short_chain = !(FEAT & F_TRI) && nops <= 2u;  // (the mesh kernels' registers are spoken for: generic path)
    if (short_chain) {
      apply_op(op0, lr);
      d0 = lr.d;
      if (nops == 2u) apply_op(op1, lr);
      d1 = lr.d;
    } else {
      lr = to_local(I, wr);
    }
  }
  const float t = b.t;
  Rec h;
  h.mat = meta.z;
  h.u = 0.0f;
  h.v = 0.0f;
  V3 outward;
  h.p = add(lr.o, scale(lr.d, t));  // ray.rs:25-27
  if (((FEAT & F_SPHERE) && type == PT_SPHERE) || ((FEAT & F_MSPHERE) && type == PT_MSPHERE)) {
    const float4 q0 = geo(0), q1 = geo(1), q2 = geo(2);
    V3 c = type == PT_SPHERE ? mk(q0.x, q0.y, q0.z) : center_at(q0, q1, PP, S.msphere_unit, lr.time);
    const float rad = q2.z;  // r (q0.w holds r * r)
    // spherical.rs:49 (p - c) / r by the corrections from RN(1 / r), computed once by the flattener (q2.w)
    // The correction keeps a zero dividend's sign only over a positive divisor (div_by_recip), and a hollow sphere's r
    // is negative: x / r = (x with r's sign folded in) / |r|, signed zeros included, so the dividend takes the sign
    // and |r|, |1 / r| divide (p.x == c.x exactly is common where the coordinates are coarse: the offset worlds)
    const V3 pc = sub(h.p, c);
    const uint32_t rs = __float_as_uint(rad) & 0x80000000u;
    const float ar = fabsf(rad), ay = fabsf(q2.w);
    const bool ok = recip_div_ok(rad);
    outward = mk(div_rcp(__uint_as_float(__float_as_uint(pc.x) ^ rs), ar, ay, ok),
                 div_rcp(__uint_as_float(__float_as_uint(pc.y) ^ rs), ar, ay, ok),
                 div_rcp(__uint_as_float(__float_as_uint(pc.z) ^ rs), ar, ay, ok));
    if ((FEAT & F_UV) && (shade_kind & (1u << 12))) sphere_uv(outward, h.u, h.v);
  } else if ((FEAT & F_TRI) && type == PT_TRI) {
    const TriUV s{b.t, b.u, b.v};  // tri_solve's values from the winning test (the same ray and operands)
    const DevTriShade& sh = S.tshade[b.prim];  // indexed like prims[] (rtw_flatten.cpp)
    float w = 1.0f - s.u - s.v;  // triangular.rs:315-323
    outward = add(add(scale(ld3(sh.n), w), scale(ld3(sh.n + 3), s.u)), scale(ld3(sh.n + 6), s.v));
    h.u = (w * sh.uv[0] + s.u * sh.uv[2]) + s.v * sh.uv[4];
    h.v = (w * sh.uv[1] + s.u * sh.uv[3]) + s.v * sh.uv[5];
  } else if ((FEAT & F_MEDIUM) && type == PT_MEDIUM) {  // volumes.rs:62-77: no face-normal logic
    outward = mk(1.0f, 0.0f, 0.0f);
  } else {
    const int axis = (int)type - PT_RECT_XY;
    const float x = axis == 2 ? h.p.y : h.p.x;
    const float y = axis == 0 ? h.p.y : h.p.z;
    const float4 q0 = geo(0);
    h.u = (x - q0.x) / (q0.y - q0.x);
    h.v = (y - q0.z) / (q0.w - q0.z);
    outward = axis == 0 ? mk(0.f, 0.f, 1.f) : (axis == 1 ? mk(0.f, 1.f, 0.f) : mk(1.f, 0.f, 0.f));
  }
  if ((FEAT & F_MEDIUM) && type == PT_MEDIUM) {
    h.n = outward;
    h.front = true;
  } else {
    face(h, lr.d, outward);
  }
  if (uni) {  // transformations.rs:29-37: p + offset, face normal against the world ray
    h.p = add(h.p, mk(S.uni_off[0], S.uni_off[1], S.uni_off[2]));
    face(h, wr.d, h.n);
  } else if ((FEAT & F_INST) && inst && short_chain) {  // unwind inner -> outer (transformations.rs:29-37, :137-147)
    auto unwind_op = [&](float4 op, V3 dk) {
      if (op_is(op.x, IO_TRANSLATE)) {
        h.p = add(h.p, mk(op.y, op.z, op.w));
        face(h, dk, h.n);
      } else {
        const float s = op.y, c = op.z;
        V3 p = mk(c * h.p.x + s * h.p.z, h.p.y, -s * h.p.x + c * h.p.z);
        V3 n = mk(c * h.n.x + s * h.n.z, h.n.y, -s * h.n.x + c * h.n.z);
        h.p = p;
        face(h, dk, n);
      }
    };
    if (nops == 2u) unwind_op(op1, d1);
    if (nops >= 1u) unwind_op(op0, d0);
  } else if ((FEAT & F_INST) && inst) {  // unwind wrappers inner -> outer (transformations.rs:29-37, :137-147)
    for (int k = (int)I->nops - 1; k >= 0; --k) {
      V3 dk = wr.d;  // direction as seen inside wrapper k = after ops 0..k
      for (int q = 0; q <= k; ++q) {
        const float4 op = *reinterpret_cast<const float4*>(I->op[q]);
        if (op_is(op.x, IO_ROTY)) dk = mk(op.z * dk.x - op.y * dk.z, dk.y, op.y * dk.x + op.z * dk.z);
      }
      const float4 op = *reinterpret_cast<const float4*>(I->op[k]);
      if (op_is(op.x, IO_TRANSLATE)) {
        h.p = add(h.p, mk(op.y, op.z, op.w));
        face(h, dk, h.n);
      } else {
        const float s = op.y, c = op.z;
        V3 p = mk(c * h.p.x + s * h.p.z, h.p.y, -s * h.p.x + c * h.p.z);
        V3 n = mk(c * h.n.x + s * h.n.z, h.n.y, -s * h.n.x + c * h.n.z);
        h.p = p;
        face(h, dk, n);
      }
    }
  }
  return h;
}

// Checker::value's decision (texture.rs:69-81) is `sinf(fx) * sinf(fy) * sinf(fz) < 0` with glibc's
// sinf.  oracle/tools/sin_sign_check.cpp proves over EVERY finite float (tests/test_checker_proof.py):
// sign(sinf x) = parity of floor(x / pi), by the double-precision product for 2^-12 <= |x| < 65536
// and by the exact integer reduction rtw::pi_parity for |x| >= 65536; sinf x == x for |x| < 2^-12;
// |sinf x| >= 3.2e-9 for |x| >= 2^-12 (no product of three such factors underflows).  So the
// decision is the XOR of the factors' signs, except that NaN / inf / 0 factors give "even" and a
// product that underflows to zero is "even".  Underflow needs a tiny factor: it is decided from the
// product of the tiny factors alone (|sin| of the others taken as 1), exact unless that product is
// below 2^-120 / 3.2e-9^k (some |f x| < ~1e-20): that corner alone is not pinned.
__device__ __forceinline__ bool checker_odd_slow(float fx, float fy, float fz) {
  const float f[3] = {fx, fy, fz};
  uint32_t neg = 0;
  float tiny = 1.0f;  // left-to-right product of the tiny factors (sinf x == x there)
#pragma unroll 1
  for (int k = 0; k < 3; ++k) {  // cold path: one copy of the reduction, not three
    const float x = f[k], ax = fabsf(x);
    if (x != x || isinf(x) || x == 0.0f) return false;  // NaN or +-0 product: `< 0` is false
    if (ax < 0x1p-12f) tiny = tiny * ax;
    neg ^= (ax < 0x1p-12f ? 0u : pi_parity(ax)) ^ (x < 0.0f ? 1u : 0u);
  }
  return neg != 0 && tiny != 0.0f;
}
__device__ __forceinline__ bool checker_odd(float fx, float fy, float fz) {
  const float ax = fabsf(fx), ay = fabsf(fy), az = fabsf(fz);
  const float lo = 0x1p-12f, hi = 65536.0f;
  if (ax >= lo && ax < hi && ay >= lo && ay < hi && az >= lo && az < hi) {
    const double INV_PI = 0.31830988618379067154;
    const int k = (int)floor((double)fx * INV_PI) + (int)floor((double)fy * INV_PI) + (int)floor((double)fz * INV_PI);
    return (k & 1) != 0;
  }
  return checker_odd_slow(fx, fy, fz);
}

// ---- Perlin noise (perlin.rs:50-122), same operation order as the oracle's perlin_noise
__device__ __forceinline__ int64_t f32_as_i64(float x) {  // Rust `as i64`: saturating, NaN -> 0
  if (x != x) return 0;
  if (x >= 9223372036854775807.0f) return INT64_MAX;
  if (x <= -9223372036854775808.0f) return INT64_MIN;
  return (int64_t)x;
}
__device__ __forceinline__ float perlin_noise(const DevPerlin& P, V3 p) {
  const V3 fl = mk(floorf(p.x), floorf(p.y), floorf(p.z));
  const uint32_t bx = (uint32_t)f32_as_i64(fl.x), by = (uint32_t)f32_as_i64(fl.y), bz = (uint32_t)f32_as_i64(fl.z);
  const V3 w = sub(p, fl);
  const V3 f = mul(mul(w, w), sub(mk(3.0f, 3.0f, 3.0f), scale(w, 2.0f)));  // filter_hermit
  float accum = 0.0f;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const uint32_t hsh = (uint32_t)P.perm[0][(bx + i) & 255u] ^ (uint32_t)P.perm[1][(by + j) & 255u] ^
                             (uint32_t)P.perm[2][(bz + k) & 255u];
        const float4 g = *reinterpret_cast<const float4*>(P.g[hsh]);
        const V3 c = mk((float)i, (float)j, (float)k);
        const V3 wv = sub(f, c);
        const V3 bl = add(mul(c, f), mul(sub(mk(1.f, 1.f, 1.f), c), sub(mk(1.f, 1.f, 1.f), f)));
        const float bf = bl.x * bl.y * bl.z;
        accum += bf * dot(mk(g.x, g.y, g.z), wv);
      }
  return accum;
}
__device__ __forceinline__ float perlin_turbulence(const DevPerlin& P, V3 p, int depth) {  // perlin.rs:78-91
  float accum = 0.0f, weight = 1.0f;
#pragma unroll 1
  for (int d = 0; d < depth; ++d) {
    accum += weight * perlin_noise(P, p);
    weight *= 0.5f;
    p = scale(p, 2.0f);
  }
  return fabsf(accum);
}

// image_texture.rs:34-52 over RGBX8 texels (rtw_flatten.cpp): one aligned 4-byte load
__device__ __forceinline__ V3 image_texel(const DevScene& S, uint32_t off, uint32_t tw, uint32_t th, float u, float v) {
  float uu = u < 0.0f ? 0.0f : (u > 1.0f ? 1.0f : u);
  float vc = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
  float vv = 1.0f - vc;
  float fi = uu * (float)tw, fj = vv * (float)th;
  uint32_t i = (fi != fi || fi <= 0.0f) ? 0u : (fi >= 4294967295.0f ? 0xFFFFFFFFu : (uint32_t)fi);
  uint32_t j = (fj != fj || fj <= 0.0f) ? 0u : (fj >= 4294967295.0f ? 0xFFFFFFFFu : (uint32_t)fj);
  i = i > tw - 1 ? tw - 1 : i;
  j = j > th - 1 ? th - 1 : j;
  const uint32_t px = *reinterpret_cast<const uint32_t*>(S.texels + off + ((size_t)j * tw + i) * 4);
  const float sc = 1.0f / 255.0f;
  return mk((float)(px & 0xffu) * sc, (float)((px >> 8) & 0xffu) * sc, (float)((px >> 16) & 0xffu) * sc);
}

// ---- textures (texture.rs:56-81, :89-104; image_texture.rs:34-52)
template <uint32_t FEAT>
__device__ V3 tex_value(const DevScene& S, uint32_t id, float u, float v, V3 p) {
  for (int guard = 0; guard < 64; ++guard) {
    const DevTex& t = S.texs[id];
    if (t.type == TT_SOLID) return ld3(t.c);
    if ((FEAT & F_CHECKER) && t.type == TT_CHECKER) {
      id = checker_odd(t.freq * p.x, t.freq * p.y, t.freq * p.z) ? t.odd : t.even;
      continue;
    }
    if ((FEAT & F_IMAGE) && t.type == TT_IMAGE) return image_texel(S, t.off, t.w, t.h, u, v);
    if ((FEAT & F_NOISE) && t.type == TT_NOISE) {  // texture.rs:89-95
      const float tb = perlin_turbulence(S.perlins[t.off], p, 7);
      const float sv = 0.5f * (1.0f + dev_sinf(t.freq * p.z + 10.0f * tb));
      return mk(sv, sv, sv);
    }
    if ((FEAT & F_UVDEBUG) && t.type == TT_UVDEBUG) return mk(u, v, 0.0f);  // UVDebug
    break;
  }
  return mk(0.f, 0.f, 0.f);
}

__device__ __forceinline__ float reflectance(float cosine, float r0) {  // material.rs:108-112, r0 precomputed (DevShade::a)
  float x = 1.0f - cosine;
  float x2 = x * x;
  return r0 + (1.0f - r0) * (x * (x2 * x2));  // powi(5) as LLVM expands it
}

// ---- the materials (material.rs:42-165, light_source.rs:17-24): one body for every material, so a wave mixing
// materials runs the rejection loop, unit() and the texture lookup once instead of once per material branch.  Each
// material's draws and f32 operations are the reference's.  In three pieces, between which a kernel draws
// rs = rand_in_unit_sphere (for lam, met and iso) and takes ud = unit(lam ? rs : d_in) itself; the throughput, the
// terminal rules and the output are each kernel's own (path_kernel, sample_kernel, scatter_kernel).
struct MatKind {
  uint32_t mode;  // DevShade's SM_*
  bool light, lam, met, iso;  // none of them: a Dielectric
};
template <uint32_t FEAT>
__device__ __forceinline__ MatKind mat_kind(uint32_t kind) {
  const uint32_t mt = kind & 0xffu;
  MatKind k;
  k.mode = (kind >> 8) & 0xfu;
  k.light = (FEAT & F_LIGHT) && mt == MT_LIGHT;
  k.lam = (FEAT & F_LAMBERT) && mt == MT_LAMBERT;
  k.met = (FEAT & F_METAL) && mt == MT_METAL;
  k.iso = (FEAT & F_ISO) && mt == MT_ISOTROPIC;
  return k;
}
// Scatter::attenuation, or a light's emission.  even(): the checker's even colour (DevShade::b), a callable so that a
// kernel short of registers can read it here, where it is used
template <uint32_t FEAT, class Even>
__device__ __forceinline__ V3 mat_attenuation(const DevScene& S, const DevShade& sh, const MatKind& k, const Rec& h,
                                              Even even) {
  V3 att = mk(1.f, 1.f, 1.f);  // Dielectric: attenuation (1,1,1)
  if (k.met) {
    att = ld3(sh.a);
  } else if (k.light || k.lam || k.iso) {
    if (k.mode == SM_SOLID) att = ld3(sh.a);  // SolidColor::value
    else if ((FEAT & F_CHECKER) && k.mode == SM_CHECKER)
      att = checker_odd(sh.param * h.p.x, sh.param * h.p.y, sh.param * h.p.z) ? ld3(sh.a) : even();
    else if ((FEAT & F_IMAGE) && k.mode == SM_IMAGE)  // (the monument's texture: no record chain)
      att = image_texel(S, __float_as_uint(sh.a[0]), __float_as_uint(sh.a[1]), __float_as_uint(sh.a[2]), h.u, h.v);
    else if (FEAT & F_TEXGEN) att = tex_value<FEAT>(S, S.mats[h.mat].tex, h.u, h.v, h.p);
  }
  return att;
}
// The scattered direction of a material that is no light; absorbed: a Metal ray below the surface (emitted() is black)
template <uint32_t FEAT>
__device__ __forceinline__ V3 mat_direction(const DevShade& sh, const MatKind& k, const Rec& h, V3 ud, V3 rs,
                                            uint64_t& rng, bool& absorbed) {
  V3 dir = rs;  // Isotropic (material.rs:155-165): never absorbs
  if (k.lam) {  // material.rs:42-56
    dir = add(h.n, ud);
    if (near_zero(dir)) dir = h.n;
  } else if (k.met) {  // material.rs:78-95
    dir = add(reflect(ud, h.n), scale(rs, sh.param));
    absorbed = !(dot(dir, h.n) > 0.0f);
  } else if (!k.iso && (FEAT & F_DIEL)) {  // Dielectric, material.rs:116-142
    // 1 / ir (material.rs:120) and Schlick's r0 (:108-112) for both ratios: the same f32
    // operations, evaluated once by the flattener (DevShade::a)
    const float ratio = h.front ? sh.a[0] : sh.param;
    const float r0 = h.front ? sh.a[1] : sh.a[2];
    const float cos_t = fminf(dot(neg(ud), h.n), 1.0f);
    const float sin_t = sqrtf(1.0f - cos_t * cos_t);
    const bool cannot = (ratio * sin_t) > 1.0f;
    if (cannot || reflectance(cos_t, r0) > gen_f32(rng)) dir = reflect(ud, h.n);
    else dir = refract(ud, h.n, ratio);
  }
  return dir;
}

}  // namespace dev
}  // namespace rtw
