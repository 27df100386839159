// rtw_dev_math.hpp — the device code's f32 arithmetic, the first header both kernel units (rtw_kernel.hip,
// rtw_kernel_mesh.hip) include: the compile-time switch fences and their #errors, the kernel constants (TMIN, BLOCK,
// STACK_*), V3, the correctly rounded sqrt, the per-path RNG and its float draws, the correctly rounded
// transcendentals, and the exact-reciprocal divisions (rcp_rn, div_rcp, unit).  Numerics: rtw_kernel.hip's header.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rtw_device.hpp"

namespace rtw {
namespace dev {

// Compile-time switches.  The product build sets none of them.  Only these remain, and none changes a
// result: RTW_NT_SAMPLES (0 = the sample buffer written / read with plain accesses; an A/B knob) and the
// COUNT-build diagnostics RTW_LANE_DIAG / RTW_UNI_DIAG (node-loop lane states) and RTW_SHADE_DIAG (shading
// sub-phase timers; each replaces the COUNT build's sub_cycles).  RTW_DIAG_ONE_TRIP (a timing diagnostic that is
// NOT the reference's distribution) refuses to compile unless RTW_ALLOW_NON_REFERENCE is set as well, so no
// product build can carry it.  Round 3's equivalence switches (sphere-root / unit() reciprocals, the
// precomputed Dielectric ratios, start_path's LDS operands, select-form rect tests) are the only code now;
// the dropped experiments (round 3's per-rect-guarded chain reciprocals, the xoroshiro64+ output) are deleted.
#if defined(RTW_DIAG_ONE_TRIP) && !defined(RTW_ALLOW_NON_REFERENCE)
#error "RTW_DIAG_ONE_TRIP changes the sampled distribution (not the reference's): diagnostic builds only"
#endif
#if defined(RTW_DIAG_FAR) && !defined(RTW_ALLOW_NON_REFERENCE)
#error "RTW_DIAG_FAR removes parts of the far-origin walk (timing diagnostic): diagnostic builds only"
#endif
#if defined(RTW_DIAG_NO_STORE) && !defined(RTW_ALLOW_NON_REFERENCE)
#error "RTW_DIAG_NO_STORE drops the sample stores (the image is not computed): diagnostic builds only"
#endif
#if defined(RTW_RNG_PLUS) || defined(RTW_RECT_RCP) || defined(RTW_SPH_RCP) || defined(RTW_FAST_RCP) || \
    defined(RTW_DIEL_PRE) || defined(RTW_START_LDS) || defined(RTW_RECT_SELECT) || defined(RTW_SRING) || \
    defined(RTW_SRING_LDSN)
#error "removed compile-time switch (round 4; round 7's start-ring A/B): the kernel has one code path for it"
#endif

constexpr float TMIN = 0.001f;  // lib.rs:102
constexpr int BLOCK = 256;
// LDS traversal-stack entries per lane (+ 1 scratch row).  At the 5 waves/SIMD the default
// variants are register-allocated for, 160 KB of LDS per CU holds 5 blocks of 256 lanes x 25 rows;
// a tree whose worst-case push bound (Flat::stack_need) is deeper keeps the excess in HBM
// (RenderArgs::spill).  STACK_LDS (33 rows) is for the 4-waves/SIMD tuning variants.
constexpr int STACK_LDS = 32;
constexpr int STACK_LDS5 = 24;
// Deep-tree variants (mesh scenes): 31 rows x 256 lanes x 4 B x 5 blocks = 158,720 B <= 160 KiB, so a
// push bound up to 30 (cow 25, monument 30) stays in LDS at 5 waves/SIMD without the spill path.
constexpr int STACK_DEEP5 = 30;

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 mk(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 mul(V3 a, V3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ V3 scale(V3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 divs(V3 a, float s) { return mk(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ V3 neg(V3 a) { return mk(-a.x, -a.y, -a.z); }
__device__ __forceinline__ float len2(V3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
// Correctly rounded f32 sqrt for x in [2^-96, inf): the backend's own expansion of sqrtf (v_sqrt_f32,
// then the +-1 ulp residual corrections) without its small-input scaling and special-value fix-up,
// which select the unscaled, uncorrected result for exactly these inputs -- the same bits, 7 fewer
// VALU ops.  tests/test_gpu_parity.py checks it against IEEE sqrt on the device.
__device__ __forceinline__ float sqrt_rn_big(float x) {
  const float s = __builtin_amdgcn_sqrtf(x);
  const float sdn = __uint_as_float(__float_as_uint(s) - 1u);
  const float sup = __uint_as_float(__float_as_uint(s) + 1u);
  const float s1 = __builtin_fmaf(-sdn, s, x) <= 0.0f ? sdn : s;
  return __builtin_fmaf(-sup, s, x) > 0.0f ? sup : s1;
}
__device__ __forceinline__ float sqrt_rn(float x) {  // = sqrtf(x) for every x
  float r = sqrt_rn_big(x);
  if (__builtin_expect(!(x >= 0x1p-96f && x < INFINITY), 0)) r = sqrtf(x);
  return r;
}
#ifndef RTW_NT_SAMPLES
#define RTW_NT_SAMPLES 1  // the sample buffer written with non-temporal stores
#endif
__device__ __forceinline__ bool near_zero(V3 a) {                                   // vec3.rs:133-138
  return fabsf(a.x) < 1e-8f && fabsf(a.y) < 1e-8f && fabsf(a.z) < 1e-8f;
}
__device__ __forceinline__ V3 reflect(V3 v, V3 n) { return sub(v, scale(n, 2.0f * dot(v, n))); }  // :140-142
__device__ __forceinline__ V3 refract(V3 uv, V3 n, float eta) {                                  // :144-151
  float cos_t = fminf(dot(neg(uv), n), 1.0f);
  V3 perp = scale(add(uv, scale(n, cos_t)), eta);
  float k = -sqrtf(fabsf(1.0f - len2(perp)));
  return add(perp, scale(n, k));
}
__device__ __forceinline__ V3 ld3(const float* p) { return mk(p[0], p[1], p[2]); }

// ---- RNG: xoroshiro64* per path (state s0 | s1 << 32, never 0) seeded by
// splitmix64(splitmix64(seed) ^ (j << 48 | i << 32 | sample)); rand 0.9 float conversions
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t xoro_seed(uint64_t h) { return h ? h : 0x9E3779B97F4A7C15ull; }
// one 32-bit multiply + 5 shift/rotate/xor ops per draw (the round-1 PCG32 step was a 64-bit
// multiply: 3 quarter-rate VALU ops)
__device__ __forceinline__ uint32_t rng_next(uint64_t& s) {
  uint32_t s0 = (uint32_t)s, s1 = (uint32_t)(s >> 32);
  const uint32_t result = s0 * 0x9E3779BBu;
  s1 ^= s0;
  s0 = __builtin_amdgcn_alignbit(s0, s0, 6) ^ s1 ^ (s1 << 9);  // rotl(s0, 26)
  s1 = __builtin_amdgcn_alignbit(s1, s1, 19);                   // rotl(s1, 13)
  s = ((uint64_t)s1 << 32) | s0;
  return result;
}
// (u >> 9) | 0x3F800000 (= 1.0f's bits: the float in [1, 2) with u's top 23 bits as mantissa) in one
// v_alignbit_b32: the low word of the 64-bit (0x7F : u) >> 9.  Inline asm: the compiler turns the builtin
// back into a shift and an or (two VALU ops per draw in the rejection loops).  AB = false keeps the shift and
// the or: the asm statement changed the triangle kernels' register allocation (MI355X A/B,
// profiles/r03/experiments r03t: jumpy +0.6%, cornell +1.0%, cow -2.4%, monument -1.2%), so only the
// sphere and list-mode kernels use it (the same split as start_path's LDS operands, SLDS).
template <bool AB>
__device__ __forceinline__ uint32_t one_mant23(uint32_t u) {
  if constexpr (!AB) return (u >> 9) | 0x3F800000u;
  uint32_t r;
  asm("v_alignbit_b32 %0, %1, %2, 9" : "=v"(r) : "s"(0x7Fu), "v"(u));
  return r;
}
__device__ __forceinline__ float gen_f32(uint64_t& s) {  // rand Standard<f32>
  return (float)(rng_next(s) >> 8) * (1.0f / 16777216.0f);
}
template <bool AB>
__device__ __forceinline__ float gen_range(uint64_t& s, float lo, float hi, float sc) {
  // UniformFloat::sample_single with sc = hi - lo precomputed (kernel-uniform: stays in an SGPR)
  for (;;) {
    float v01 = __uint_as_float(one_mant23<AB>(rng_next(s))) - 1.0f;
    float r = v01 * sc + lo;
    if (r < hi) return r;
    sc = __uint_as_float(__float_as_uint(sc) - 1u);
  }
}
// gen_range(s, -1, 1) without the retry loop: v12 = 1 + m 2^-23 (m < 2^23), and
// (v12 - 1) * 2 + -1 = 2 v12 - 3 = (m - 2^22) 2^-22 is exact in both forms and at most 1 - 2^-22 < 1,
// so the retry never fires (checked for every m in tests/test_oracle_kat.py::test_pm1_never_retries)
// and one exact fma gives the oracle's bits.
template <bool AB>
__device__ __forceinline__ float gen_pm1(uint64_t& s) {
  const float v12 = __uint_as_float(one_mant23<AB>(rng_next(s)));
  return __builtin_fmaf(v12, 2.0f, -3.0f);
}
template <bool AB>
__device__ __forceinline__ V3 rand_in_unit_sphere(uint64_t& s) {  // vec3.rs:101-108
  for (;;) {
    float x = gen_pm1<AB>(s);
    float y = gen_pm1<AB>(s);
    float z = gen_pm1<AB>(s);
    V3 p = mk(x, y, z);
#ifdef RTW_DIAG_ONE_TRIP  // timing diagnostic only (not the reference's distribution): no rejection tail
    return p;
#endif
    if (len2(p) < 1.0f) return p;
  }
}
template <bool AB>
__device__ __forceinline__ V3 rand_in_unit_disk(uint64_t& s) {  // vec3.rs:124-131
  for (;;) {
    float x = gen_pm1<AB>(s);
    float y = gen_pm1<AB>(s);
    V3 p = mk(x, y, 0.0f);
    if (len2(p) < 1.0f) return p;
  }
}

// ---- f32 transcendentals, correctly rounded: evaluated in double with polynomials of error
// < 2^-60 and rounded once (the oracle's §libm restates the same algorithm; tests pin GPU ==
// oracle == (float)glibc-double).  Only IEEE double + - * / sqrt floor: no FMA contraction
// (-ffp-contract=off), so the bits are the oracle's.
__device__ __forceinline__ double ln_core(double m) {  // 2 atanh((m-1)/(m+1)), m in [sqrt(1/2), sqrt(2)]
  const double s = (m - 1.0) / (m + 1.0), z = s * s;
  double p = 1.0 / 23.0;
  p = p * z + 1.0 / 21.0; p = p * z + 1.0 / 19.0; p = p * z + 1.0 / 17.0; p = p * z + 1.0 / 15.0;
  p = p * z + 1.0 / 13.0; p = p * z + 1.0 / 11.0; p = p * z + 1.0 / 9.0; p = p * z + 1.0 / 7.0;
  p = p * z + 1.0 / 5.0; p = p * z + 1.0 / 3.0; p = p * z + 1.0;
  return 2.0 * s * p;
}
__device__ __forceinline__ float dev_log10f(float x) {  // f32::log10
  if (x != x) return x;
  if (x == 0.0f) return -INFINITY;
  if (x < 0.0f) return NAN;
  if (isinf(x)) return x;
  const uint64_t u = (uint64_t)__double_as_longlong((double)x);
  int e = (int)((u >> 52) & 0x7ff) - 1023;
  double m = __longlong_as_double((long long)((u & 0x000fffffffffffffull) | 0x3ff0000000000000ull));
  if (m > 1.4142135623730951) { m = m * 0.5; e = e + 1; }
  const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
  const double INV_LN10 = 0.43429448190325182765;
  const double lnx = ((double)e * LN2_HI + ln_core(m)) + (double)e * LN2_LO;
  return (float)(lnx * INV_LN10);
}
__device__ __forceinline__ double sin_core(double r) {
  const double z = r * r;
  double p = -1.0 / 1307674368000.0;
  p = p * z + 1.0 / 6227020800.0; p = p * z - 1.0 / 39916800.0; p = p * z + 1.0 / 362880.0;
  p = p * z - 1.0 / 5040.0; p = p * z + 1.0 / 120.0; p = p * z - 1.0 / 6.0;
  return r + r * z * p;
}
__device__ __forceinline__ double cos_core(double r) {
  const double z = r * r;
  double p = 1.0 / 20922789888000.0;
  p = p * z - 1.0 / 87178291200.0; p = p * z + 1.0 / 479001600.0; p = p * z - 1.0 / 3628800.0;
  p = p * z + 1.0 / 40320.0; p = p * z - 1.0 / 720.0; p = p * z + 1.0 / 24.0; p = p * z - 0.5;
  return 1.0 + z * p;
}
__device__ __forceinline__ float dev_sinf(float x) {  // f32::sin
  if (x != x || x == 0.0f) return x;  // keeps the sign of zero
  if (isinf(x)) return NAN;
  const double d = x;
  const double TWO_OVER_PI = 6.36619772367581382433e-01;
  const double P1 = 1.57079632673412561417e+00, P2 = 6.07710050650619224932e-11, P3 = 2.02226624879595063154e-21;
  const double k = floor(d * TWO_OVER_PI + 0.5);
  const double r = ((d - k * P1) - k * P2) - k * P3;
  const double q = k - 4.0 * floor(k * 0.25);
  const double v = q == 0.0 ? sin_core(r) : (q == 1.0 ? cos_core(r) : (q == 2.0 ? -sin_core(r) : -cos_core(r)));
  return (float)v;
}
__device__ __forceinline__ double atan_core(double t) {  // |t| <= tan(pi/16)
  const double z = t * t;
  double p = -1.0 / 29.0;
  p = p * z + 1.0 / 27.0; p = p * z - 1.0 / 25.0; p = p * z + 1.0 / 23.0; p = p * z - 1.0 / 21.0;
  p = p * z + 1.0 / 19.0; p = p * z - 1.0 / 17.0; p = p * z + 1.0 / 15.0; p = p * z - 1.0 / 13.0;
  p = p * z + 1.0 / 11.0; p = p * z - 1.0 / 9.0; p = p * z + 1.0 / 7.0; p = p * z - 1.0 / 5.0;
  p = p * z + 1.0 / 3.0;
  return t - t * z * p;
}
__device__ __forceinline__ double atan01(double a) {  // 0 <= a <= 1
  const double T1 = 0.19891236737965800691, T3 = 0.66817863791929891999, C1 = 0.41421356237309504880;
  const double PI_8 = 0.39269908169872415481, PI_4 = 0.78539816339744830962;
  if (a <= T1) return atan_core(a);
  if (a <= T3) return PI_8 + atan_core((a - C1) / (1.0 + a * C1));
  return PI_4 + atan_core((a - 1.0) / (1.0 + a));
}
__device__ __forceinline__ double atan2_pos(double y, double x) {  // y > 0 finite, x finite non-zero
  const double PI = 3.14159265358979323846, PI_2 = 1.57079632679489661923;
  const double ax = fabs(x);
  const double r = y <= ax ? atan01(y / ax) : PI_2 - atan01(ax / y);
  return x < 0.0 ? PI - r : r;
}
__device__ __forceinline__ float dev_atan2f(float y, float x) {  // f32::atan2, C99 Annex F special cases
  const double PI = 3.14159265358979323846, PI_2 = 1.57079632679489661923, PI_4 = 0.78539816339744830962;
  if (x != x || y != y) return x + y;
  const bool sx = signbit(x), sy = signbit(y);
  double r;
  if (y == 0.0f) r = sx ? PI : 0.0;
  else if (isinf(x)) r = isinf(y) ? (sx ? 3.0 * PI_4 : PI_4) : (sx ? PI : 0.0);
  else if (x == 0.0f || isinf(y)) r = PI_2;
  else r = atan2_pos(fabs((double)y), (double)x);
  return (float)(sy ? -r : r);
}
__device__ __forceinline__ float dev_acosf(float x) {  // f32::acos = atan2(sqrt((1-x)(1+x)), x)
  if (x != x) return x;
  if (!(fabsf(x) <= 1.0f)) return NAN;
  const double d = x, s = sqrt((1.0 - d) * (1.0 + d));
  if (s == 0.0) return d > 0.0 ? 0.0f : (float)3.14159265358979323846;
  return (float)atan2_pos(s, d);
}

// RN(x / b) from y = RN(1 / b) by Markstein's correction (q0 = RN(x y) is within an ulp of x / b, the
// residual r = x - q0 b is exact in one fma, and RN(q0 + r y) = RN(x / b); Markstein 1990, no
// underflow or overflow): the camera's u, v divisions (lib.rs:84-85), whose divisors w - 1, h - 1 are
// integers in [1, 65535] and dividends 0 or in [2^-24, 65536), with y computed exactly on the host.
// Three VALU ops instead of the ~10 of an IEEE division; tests/test_gpu_parity.py checks it against
// IEEE division on the device.
// The residual is formed negated, t = q0 b - x = -r, and taken off again: the same roundings for every x != 0 (fma
// rounds to nearest, which is symmetric), the same three VALU ops (the negations are source modifiers), and over a
// positive divisor -- a length in unit(), w - 1 and h - 1 in the camera -- a zero x keeps its sign as an IEEE quotient
// does.  With r = fma(-q0, b, x) a dividend of -0 gave q0 = -0, r = +0 + -0 = +0 and fma(+0, y, -0) = +0: unit() turned
// a direction component of -0 into +0, which Metal's and the Dielectric's reflected rays then carried
// (tests/test_gpu_ray_corpus.py::test_unit_keeps_the_sign_of_a_zero_component).  Over a negative divisor a dividend of
// +0 gives +0 where IEEE gives -0 (no three-op form is right for both signs of b: the residual of a zero dividend is
// +0 whatever its sign).  So the hit record's (p - c) / r, whose r is negative for a hollow sphere, divides by |r| with
// r's sign folded into the dividend (rtw_dev_shade.hpp); the rect test, the other signed divisor, rejects t = +-0
// alike, below t_min.
__device__ __forceinline__ float div_by_recip(float x, float b, float y) {
  const float q0 = x * y;
  const float t = __builtin_fmaf(q0, b, -x);
  return __builtin_fmaf(-t, y, q0);
}
// RN(1 / b) in three VALU ops: the hardware reciprocal (v_rcp_f32, within 1 ulp) refined by one Newton
// step with an exact residual, e = 1 - b y0 (fma), y1 = RN(y0 + e y0).  Equal to the IEEE quotient 1.0f / b
// for every b with |b| in [2^-126, 2^126] (normal b whose reciprocal is normal): checked on the device over
// all 2^32 bit patterns (rtw_diag_sweep 0, tests/test_gpu_parity.py), which is the proof, since v_rcp_f32
// is a fixed function of its input.  Callers guard the range (rcp_rn_ok) and divide otherwise.
__device__ __forceinline__ float rcp_rn_fast(float b) {
  const float y0 = __builtin_amdgcn_rcpf(b);
  const float e = __builtin_fmaf(-b, y0, 1.0f);
  return __builtin_fmaf(e, y0, y0);
}
__device__ __forceinline__ bool rcp_rn_ok(float b) {
  const float ab = fabsf(b);
  return ab >= 0x1p-126f && ab <= 0x1p126f;
}
__device__ __forceinline__ float rcp_rn(float b) {  // = 1.0f / b for every b
  float y = rcp_rn_fast(b);
  if (__builtin_expect(!rcp_rn_ok(b), 0)) y = 1.0f / b;
  return y;
}
// RN(x / b) from y = RN(1 / b) with the range guard of the sphere roots: Markstein's correction is the IEEE
// quotient wherever b is in [2^-60, 2^60] and |x| < 2^64 and the quotient is normal, and below 2^-126 both
// are tiny (< TMIN); other lanes divide.
__device__ __forceinline__ bool recip_div_ok(float b) {
  const float ab = fabsf(b);
  return ab >= 0x1p-60f && ab <= 0x1p60f;
}
__device__ __forceinline__ float div_rcp(float x, float b, float y, bool b_ok) {
  float t = div_by_recip(x, b, y);
  if (__builtin_expect(!(b_ok && fabsf(x) < 0x1p64f), 0)) t = x / b;
  return t;
}
// vec3.rs:85-87 unit_vector: a / |a|.  |a| = sqrt_rn (IEEE sqrt); the three divisions share the divisor, so
// one rcp_rn and three corrections; |a.k| <= |a| needs no numerator guard.
__device__ __forceinline__ V3 unit(V3 a) {
  const float s = sqrt_rn(len2(a));
  const float y = rcp_rn_fast(s);
  V3 r = mk(div_by_recip(a.x, s, y), div_by_recip(a.y, s, y), div_by_recip(a.z, s, y));
  if (__builtin_expect(!recip_div_ok(s), 0)) r = divs(a, s);
  return r;
}

}  // namespace dev
}  // namespace rtw
