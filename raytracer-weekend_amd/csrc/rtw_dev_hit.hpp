// rtw_dev_hit.hpp — one ray against one thing: Ray, the scalar table loads (uload), the wrapper chains (to_local),
// every primitive's candidate t (cand_*), the closest-hit fold (Best: min t, ties to the larger DFS key), constant
// media, the sphere / primitive / triangle-leaf tests the walks call, and the BVH slab test.
#pragma once
#include "rtw_dev_math.hpp"

namespace rtw {
namespace dev {

struct Ray { V3 o, d; float time; };

// ---- wrapper chains (transformations.rs:23-38, :115-135): world ray -> object ray
// Wave-uniform loads of scene tables through the constant address space: the backend emits scalar
// loads (s_load, scalar cache) instead of 64-lane vector loads of one address, which kept the
// vector-memory units of the list-mode kernel busy (cornell-box: TA 94%, TD 99%).  Reads only: the
// kernel never writes the scene tables.
template <class T>
__device__ __forceinline__ T uload(const T* p) {
  if constexpr (sizeof(T) == 16) {  // HIP vector types: load the native 4 x 32-bit vector
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const u4 v = *(const __attribute__((address_space(4))) u4*)(p);
    T t;
    __builtin_memcpy(&t, &v, 16);
    return t;
  } else {
    return *(const __attribute__((address_space(4))) T*)(p);
  }
}

// a wrapper op's kind (op.x holds (float)IO_TRANSLATE or (float)IO_ROTY, rtw_flatten.cpp) compared as bits: an
// integer compare, which a kernel-uniform op does on the scalar unit (a float compare is a VALU op plus an exec and)
__device__ __forceinline__ bool op_is(float x, uint32_t kind) { return __float_as_uint(x) == __float_as_uint((float)kind); }

template <bool UNI = false>
__device__ __forceinline__ Ray to_local(const DevInst* in, Ray r) {
  const uint32_t n = UNI ? uload(&in->nops) : in->nops;
  for (uint32_t k = 0; k < n; ++k) {
    const float4* opp = reinterpret_cast<const float4*>(in->op[k]);
    const float4 op = UNI ? uload(opp) : *opp;
    if (op_is(op.x, IO_TRANSLATE)) {
      r.o = sub(r.o, mk(op.y, op.z, op.w));
    } else {
      const float s = op.y, c = op.z;
      r.o = mk(c * r.o.x - s * r.o.z, r.o.y, s * r.o.x + c * r.o.z);
      r.d = mk(c * r.d.x - s * r.d.z, r.d.y, s * r.d.x + c * r.d.z);
    }
  }
  return r;
}

// ---- candidate t of one primitive (independent of t_max; -1 = miss)
// rad2 = radius * radius (precomputed for moving spheres; the same f32 product)
__device__ __forceinline__ float cand_sphere(const Ray& r, V3 c, float rad2) {  // spherical.rs:26-44
  V3 oc = sub(r.o, c);
  float a = len2(r.d);
  float hb = dot(oc, r.d);
  float cc = len2(oc) - rad2;
  float disc = hb * hb - a * cc;
  if (disc < 0.0f) return -1.0f;  // spherical.rs:32: a NaN discriminant goes on (a NaN root, a hit in list mode)
  float sq = sqrtf(disc);
  float root = (-hb - sq) / a;
  if (root < TMIN) root = (-hb + sq) / a;  // root1 > t_max implies root2 > t_max
  return root;
}
// The same test with the ray's a = |d|^2 and y = RN(1 / a) computed once per traversal (SphRcp): each
// root is Markstein's correction div_by_recip (3 VALU) instead of an IEEE division (~10).  Equal to
// the IEEE quotient whenever a is in [2^-60, 2^60] and |numerator| < 2^64 (then the quotient is finite,
// and wherever it is normal the correction is exact; below 2^-126 both are < TMIN); other lanes divide.
struct SphRcp { float a, ya; bool ok; };
__device__ __forceinline__ SphRcp sph_rcp(const Ray& r) {
  SphRcp q;
  q.a = len2(r.d);
  q.ya = rcp_rn_fast(q.a);  // = 1.0f / a inside the guarded range below (outside it sph_div divides)
  q.ok = q.a >= 0x1p-60f && q.a <= 0x1p60f;
  return q;
}
__device__ __forceinline__ float sph_div(float n, const SphRcp& q) {
  float t = div_by_recip(n, q.a, q.ya);
  if (__builtin_expect(!(q.ok && fabsf(n) < 0x1p64f), 0)) t = n / q.a;
  return t;
}
__device__ __forceinline__ float cand_sphere_rcp(const Ray& r, V3 c, float rad2, const SphRcp& q) {
  V3 oc = sub(r.o, c);
  float hb = dot(oc, r.d);
  float cc = len2(oc) - rad2;
  float disc = hb * hb - q.a * cc;
  if (!(disc >= 0.0f)) return -1.0f;
  float sq = sqrt_rn(disc);
  float root = sph_div(-hb - sq, q);
  if (root < TMIN) root = sph_div(-hb + sq, q);
  return root;
}
// spherical.rs:117-123 over the flattened layout q0 = (c0, r*r), q1 = (c1 - c0, r), q2 = (t0, t1)
// (rtw_flatten.cpp).  For the shutter [+0, 1] (aux = 1) the fraction (time - 0) / (1 - 0) is `time`
// exactly: when every moving sphere of the scene has it (DevScene::msphere_unit, a kernel-uniform
// branch) the IEEE division and the q2 load are skipped; otherwise each prim's t0, t1 are used.
__device__ __forceinline__ V3 center_at(float4 q0, float4 q1, const float4* P, uint32_t unit_shutter, float time) {
  float frac = time;
  if (!unit_shutter) {
    const float4 q2 = P[2];
    frac = (time - q2.x) / (q2.y - q2.x);
  }
  return add(mk(q0.x, q0.y, q0.z), scale(mk(q1.x, q1.y, q1.z), frac));
}
template <int AXIS, bool SEL = false>  // 0 XY, 1 XZ, 2 YZ — rectangular.rs:33-41, :84-92, :135-143
__device__ __forceinline__ float cand_rect(const Ray& r, const float* q0, float k) {
  const float o_k = AXIS == 0 ? r.o.z : (AXIS == 1 ? r.o.y : r.o.x);
  const float d_k = AXIS == 0 ? r.d.z : (AXIS == 1 ? r.d.y : r.d.x);
  const float o_a = AXIS == 2 ? r.o.y : r.o.x, d_a = AXIS == 2 ? r.d.y : r.d.x;
  const float o_b = AXIS == 0 ? r.o.y : r.o.z, d_b = AXIS == 0 ? r.d.y : r.d.z;
  float t = (k - o_k) / d_k;
  if constexpr (SEL) {
    // the same decisions as selects (x, y have no side effects): no exec-mask branches in the list loop
    const float x = o_a + t * d_a;
    const float y = o_b + t * d_b;
    const bool out = (t < TMIN) | (x < q0[0]) | (x > q0[1]) | (y < q0[2]) | (y > q0[3]);
    return out ? -1.0f : t;
  }
  if (t < TMIN) return -1.0f;
  float x = o_a + t * d_a;
  float y = o_b + t * d_b;
  if (x < q0[0] || x > q0[1] || y < q0[2] || y > q0[3]) return -1.0f;
  return t;
}
struct TriUV { float t, u, v; };
__device__ __forceinline__ TriUV tri_solve(const Ray& r, const float* q) {  // triangular.rs:98-118
  V3 a = mk(q[0], q[1], q[2]), ab = mk(q[3], q[4], q[5]), ac = mk(q[6], q[7], q[8]);
  V3 n = mk(q[9], q[10], q[11]);
  float det = -dot(r.d, n);
  float inv = rcp_rn(det);  // triangular.rs:105 `1.0 / determinant`, the IEEE reciprocal
  V3 ao = sub(r.o, a);
  V3 aoxd = cross(ao, r.d);
  TriUV o;
  o.u = dot(ac, aoxd) * inv;
  o.v = -dot(ab, aoxd) * inv;
  o.t = dot(ao, n) * inv;
  return o;
}
__device__ __forceinline__ float cand_tri(const Ray& r, const float* q) {
  TriUV s = tri_solve(r, q);
  if (s.t < TMIN) return -1.0f;
  if (!(s.t >= 0.0f && s.u >= 0.0f && s.v >= 0.0f && (s.u + s.v) <= 1.0f)) return -1.0f;
  return s.t;
}
__device__ __forceinline__ float cand_tri_uv(const Ray& r, const float* q, float& u, float& v) {
  TriUV s = tri_solve(r, q);
  u = s.u;
  v = s.v;
  if (s.t < TMIN) return -1.0f;
  if (!(s.t >= 0.0f && s.u >= 0.0f && s.v >= 0.0f && (s.u + s.v) <= 1.0f)) return -1.0f;
  return s.t;
}

struct Best {
  float t;
  uint32_t key;
  int32_t prim;
  float u, v;  // a triangle winner's barycentrics (tri_solve's, triangular.rs:109-112): the hit record reuses them
};

// ConstantMedium::hit (volumes.rs:37-78) in the order-independent form the oracle defines (K_MEDIUM):
// boundary entry / exit by the reference's own hit routines with t in (-inf, inf) and
// (rec1 + 0.0001, inf), distance test against the unclipped exit, and the draw from a sub-stream
// keyed by (segment state, leaf key).  -1 = no hit.
template <uint32_t FEAT>
__device__ __forceinline__ float cand_medium(const DevScene& S, const Ray& lr, const float4* P, uint32_t key,
                                          uint32_t inner, uint64_t seg) {
  const float4 q0v = P[0], q1v = P[1], q2v = P[2];
  const Ray br = ((FEAT & F_INST) && inner) ? to_local(S.insts + inner, lr) : lr;
  float r1, r2;
  if (q2v.y == 0.0f) {  // Sphere boundary: spherical.rs:18-60 twice
    const V3 oc = sub(br.o, mk(q0v.x, q0v.y, q0v.z));
    const float a = len2(br.d), hb = dot(oc, br.d), cc = len2(oc) - q0v.w * q0v.w;
    const float disc = hb * hb - a * cc;
    if (disc < 0.0f) return -1.0f;
    const float sq = sqrtf(disc);
    const float root1 = (-hb - sq) / a, root2 = (-hb + sq) / a;
    float rt = root1;
    if (rt < -INFINITY || INFINITY < rt) {
      rt = root2;
      if (rt < -INFINITY || INFINITY < rt) return -1.0f;
    }
    r1 = rt;
    const float lo = r1 + 0.0001f;
    rt = root1;
    if (rt < lo || INFINITY < rt) {
      rt = root2;
      if (rt < lo || INFINITY < rt) return -1.0f;
    }
    r2 = rt;
  } else {  // Cuboid boundary: its six rects (rectangular.rs:177-240) as a closest-hit list, twice
    const float p0[3] = {q0v.x, q0v.y, q0v.z}, p1[3] = {q1v.x, q1v.y, q1v.z};
    const float o[3] = {br.o.x, br.o.y, br.o.z}, d[3] = {br.d.x, br.d.y, br.d.z};
    float ts[6];
    bool inb[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int axis = k >> 1;  // XY, XY, XZ, XZ, YZ, YZ; k on z / y / x, far side first
      const int kx = axis == 0 ? 2 : (axis == 1 ? 1 : 0), ax = axis == 2 ? 1 : 0, bx = axis == 0 ? 1 : 2;
      const float kk = (k & 1) ? p0[kx] : p1[kx];
      const float t = (kk - o[kx]) / d[kx];
      const float x = o[ax] + t * d[ax], y = o[bx] + t * d[bx];
      ts[k] = t;
      inb[k] = !(x < p0[ax] || x > p1[ax] || y < p0[bx] || y > p1[bx]);
    }
    float closest = INFINITY;
    bool any = false;
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (inb[k] && !(ts[k] < -INFINITY || ts[k] > closest)) { closest = ts[k]; any = true; }
    if (!any) return -1.0f;
    r1 = closest;
    const float lo = r1 + 0.0001f;
    closest = INFINITY;
    any = false;
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (inb[k] && !(ts[k] < lo || ts[k] > closest)) { closest = ts[k]; any = true; }
    if (!any) return -1.0f;
    r2 = closest;
  }
  float t1 = fmaxf(r1, TMIN);
  if (t1 >= r2) return -1.0f;
  t1 = fmaxf(t1, 0.0f);
  const float len = sqrtf(len2(lr.d));
  const float dist = (r2 - t1) * len;
  uint64_t g = xoro_seed(splitmix64(seg ^ splitmix64((uint64_t)key)));
  const float hd = q2v.x * dev_log10f(gen_f32(g));
  if (hd > dist) return -1.0f;
  return t1 + hd / len;
}

// COUNT build only: wave-level SIMD utilisation.  Adds 1 to cnt[wave_slot] for the first
// active lane (one per wave execution) and the wave's active-lane count to cnt[lane_slot].
__device__ __forceinline__ void simd_tick(uint32_t* cnt, int wave_slot, int lane_slot) {
  const uint64_t m = __ballot(1);
  if ((uint32_t)__lane_id() == (uint32_t)(__ffsll((long long)m) - 1)) {
    cnt[wave_slot] += 1;
    cnt[lane_slot] += (uint32_t)__popcll(m);
  }
}

// The sphere-only kernels' branch-free 32-B test (q0 = (c0, r^2), q1 = (c1 - c0, key bits); see test_prim)
__device__ __forceinline__ void test_sphere32(const DevScene& S, uint32_t pi, float4 q0v, float4 q1v, const Ray& wr,
                                              Best& b, const SphRcp* rq) {
  const float4* P = reinterpret_cast<const float4*>(S.prims + pi);
  const V3 c = center_at(q0v, q1v, P, S.msphere_unit, wr.time);
  const float t = rq ? cand_sphere_rcp(wr, c, q0v.w, *rq) : cand_sphere(wr, c, q0v.w);
  const uint32_t key = __float_as_uint(q1v.w);
  if (t >= TMIN && t < INFINITY && (t < b.t || (t == b.t && key > b.key))) {
    b.t = t;
    b.key = key;
    b.prim = (int32_t)pi;
  }
}

// List-mode kernels (F_LIST): a winner whose t is NaN (an in-plane hit, see rect_list_test) is carried with best
// t = +inf and this bit in its index (list worlds have few prims); trace_begin hands it on with t = NaN
constexpr int32_t RECT_NAN_HIT = 0x40000000;

// LOCAL: `wr` already is the prim's object-space ray (the caller caches it per wrapper chain)
// UNI: pi is wave-uniform (the always list): scalar loads (uload)
template <bool COUNT, uint32_t FEAT, bool LOCAL = false, bool UNI = false>
__device__ __forceinline__ void test_prim(const DevScene& S, uint32_t pi, const Ray& wr, Best& b,
                                          uint32_t* cnt, uint64_t seg, const SphRcp* rq = nullptr) {
  const float4* P = reinterpret_cast<const float4*>(S.prims + pi);
  // sphere-only worlds: a static sphere is tested as a moving one with c1 - c0 = 0 (c0 + time * 0 is
  // c0 up to the sign of a zero coordinate, which changes neither the decision nor t: the zero only
  // reaches hb, whose sign matters only when every term and sqrt(disc) vanish, a root of +-0 that
  // fails t >= 0.001 either way), so one branch-free test reads q0 = (c0, r^2) and q1 = (c1 - c0,
  // key bits) -- 32 B, no type dispatch
  constexpr bool SPH_ONLY = (FEAT & (F_RECT | F_TRI | F_MEDIUM | F_INST)) == 0 && (FEAT & (F_SPHERE | F_MSPHERE));
  if constexpr (SPH_ONLY && !COUNT) {
    const float4 q0v = UNI ? uload(P) : P[0];
    const float4 q1v = UNI ? uload(P + 1) : P[1];
    test_sphere32(S, pi, q0v, q1v, wr, b, rq);
    return;
  }
  // every 16-B part the scene's primitive kinds may need is loaded up front, in one round trip:
  // loading the geometry only after the type was known cost two more dependent trips per test
  const uint4 meta = UNI ? uload(reinterpret_cast<const uint4*>(P + 3)) : *reinterpret_cast<const uint4*>(P + 3);
  const float4 q0v = UNI ? uload(P) : P[0];
  constexpr bool NEED_Q1 = (FEAT & (F_MSPHERE | F_TRI | F_RECT)) != 0, NEED_Q2 = (FEAT & F_TRI) != 0;
  const float4 q1v = NEED_Q1 ? (UNI ? uload(P + 1) : P[1]) : q0v;
  const float4 q2v = NEED_Q2 ? (UNI ? uload(P + 2) : P[2]) : q0v;
  const uint32_t type = meta.x & 0xffu, inst = meta.x >> 8;
  // rect tests and the accept as selects instead of exec-mask branches (RTW_RECT_SELECT) in the kernels
  // without triangles: cornell-800 +6.7%; the triangle kernels lost 0.6-1.4% (profiles/r03/experiments, u1)
  constexpr bool SEL = !(FEAT & F_TRI);
  // object-space ray of the prim's wrapper chain; in BVH leaves recomputed per test (a few
  // flops) rather than cached, which keeps 8 VGPRs free for occupancy
  Ray lr = wr;
  if (!LOCAL && (FEAT & F_INST) && inst) {
    if (inst == S.uni_inst)  // transformations.rs:23-38 with the kernel-uniform offset: no dependent loads
      lr.o = sub(wr.o, mk(S.uni_off[0], S.uni_off[1], S.uni_off[2]));
    else
      lr = to_local<UNI>(S.insts + inst, wr);
  }
  float q0[4] = {q0v.x, q0v.y, q0v.z, q0v.w};
  float t = -1.0f, tu = 0.0f, tv = 0.0f;
  if ((FEAT & F_SPHERE) && type == PT_SPHERE) {
    t = cand_sphere(lr, mk(q0[0], q0[1], q0[2]), q0[3]);  // q0.w = r * r (flattener, the same f32 product)
  } else if ((FEAT & F_MSPHERE) && type == PT_MSPHERE) {
    t = cand_sphere(lr, center_at(q0v, q1v, P, S.msphere_unit, lr.time), q0v.w);
  } else if ((FEAT & F_TRI) && type == PT_TRI) {
    const float q[12] = {q0v.x, q0v.y, q0v.z, q0v.w, q1v.x, q1v.y, q1v.z, q1v.w, q2v.x, q2v.y, q2v.z, q2v.w};
    t = cand_tri_uv(lr, q, tu, tv);
  } else if ((FEAT & F_MEDIUM) && type == PT_MEDIUM) {
    t = cand_medium<FEAT>(S, lr, P, meta.y, meta.w, seg);
  } else if (FEAT & F_RECT) {
    const float k = q1v.x;
    if (type == PT_RECT_XY) t = cand_rect<0, SEL>(lr, q0, k);
    else if (type == PT_RECT_XZ) t = cand_rect<1, SEL>(lr, q0, k);
    else if (type == PT_RECT_YZ) t = cand_rect<2, SEL>(lr, q0, k);
  }
  if (COUNT) { cnt[1]++; if (type < 6u) cnt[2 + type]++; simd_tick(cnt, 10, 11); }  // media: total only
  if constexpr ((FEAT & F_LIST) != 0) {
    // list mode tests in DFS-key order: the reference's own fold (hittable/mod.rs:57-69) with its comparisons,
    // which a NaN candidate passes (rectangular.rs:33-41, spherical.rs:32-43): best NaN behaves as best +inf
    // (RECT_NAN_HIT); a later object wins ties by order
    const bool acc = !(t < TMIN) & !(t > b.t);
    const bool tnan = t != t;
    b.t = acc ? (tnan ? INFINITY : t) : b.t;
    b.key = acc ? meta.y : b.key;
    b.prim = acc ? ((int32_t)pi | (tnan ? RECT_NAN_HIT : 0)) : b.prim;
    if (FEAT & F_TRI) {
      b.u = acc ? tu : b.u;
      b.v = acc ? tv : b.v;
    }
    return;
  }
  // hittable/mod.rs:61-65: accept t <= closest_so_far; a later object (larger key) wins ties
  if constexpr (SEL) {
    const bool acc = (t >= TMIN) & (t < INFINITY) & ((t < b.t) | ((t == b.t) & (meta.y > b.key)));
    b.t = acc ? t : b.t;
    b.key = acc ? meta.y : b.key;
    b.prim = acc ? (int32_t)pi : b.prim;
  } else if (t >= TMIN && t < INFINITY && (t < b.t || (t == b.t && meta.y > b.key))) {
    b.t = t;
    b.key = meta.y;
    b.prim = (int32_t)pi;
    if (FEAT & F_TRI) {
      b.u = tu;
      b.v = tv;
    }
  }
}

// A BVH leaf triangle when every leaf is a triangle of one wrapper chain (DevScene::bvh_tri): `lr` is
// already the chain's object-space ray, no type dispatch; the 48 B of geometry in three loads, and the
// tie key (DevPrim::key) only for a candidate at or below the best t (triangular.rs:97-138).
template <bool COUNT>
__device__ __forceinline__ void test_tri_leaf(const DevScene& S, uint32_t pi, const Ray& lr, Best& b, uint32_t* cnt) {
  const float4* P = reinterpret_cast<const float4*>(S.prims + pi);
  const float4 q0v = P[0], q1v = P[1], q2v = P[2];
  const float q[12] = {q0v.x, q0v.y, q0v.z, q0v.w, q1v.x, q1v.y, q1v.z, q1v.w, q2v.x, q2v.y, q2v.z, q2v.w};
  float u, v;
  const float t = cand_tri_uv(lr, q, u, v);
  if (COUNT) { cnt[1]++; cnt[2 + PT_TRI]++; simd_tick(cnt, 10, 11); }
  if (t >= TMIN && t < INFINITY && t <= b.t) {  // hittable/mod.rs:61-65, the key read only here
    const uint32_t key = reinterpret_cast<const uint4*>(P + 3)->y;
    if (t < b.t || key > b.key) {
      b.t = t;
      b.key = key;
      b.prim = (int32_t)pi;
      b.u = u;
      b.v = v;
    }
  }
}

// Conservative slab test on a padded box (culling only; never decides a hit).
__device__ __forceinline__ bool slab_test(float lx, float ly, float lz, float hx, float hy, float hz,
                                          V3 inv, V3 ood, float tmax_c, float& tnear) {
  float tx0 = __builtin_fmaf(lx, inv.x, -ood.x), tx1 = __builtin_fmaf(hx, inv.x, -ood.x);
  float ty0 = __builtin_fmaf(ly, inv.y, -ood.y), ty1 = __builtin_fmaf(hy, inv.y, -ood.y);
  float tz0 = __builtin_fmaf(lz, inv.z, -ood.z), tz1 = __builtin_fmaf(hz, inv.z, -ood.z);
  float tn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), 0.0f));
  float tf = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fminf(fmaxf(tz0, tz1), tmax_c));
  tnear = tn;
  return tn <= tf;
}

}  // namespace dev
}  // namespace rtw
