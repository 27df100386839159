// rtw_dev_trace.hpp — the closest-hit query of [Box<dyn Hittable>]::hit (hittable/mod.rs:57-69): TraceState, the
// list-mode rect loop, the far-origin walk (trace_far), trace_begin (the always-tested list; every primitive in list
// mode) and trace_run, the resumable 4-wide BVH walk with postponed leaves in its 32-bit, 16-bit (S16) and LDS-node
// forms.
#pragma once
#include "rtw_dev_hit.hpp"

namespace rtw {
namespace dev {

// Resumable closest-hit query.  A traversal can be suspended between two leaf phases and
// resumed in a later iteration of the path loop, so a wave does not wait for its slowest ray:
// trace_run returns as soon as `quota` lanes are done and the rest continue next time.
struct TraceState {
  Best b;
  int32_t node;  // node4 to visit next, -1 = none
  int32_t pend;  // parked leaf word ~(first << 3 | count), 0 = none
  int32_t sp;    // LDS stack depth
  bool on;       // a traversal is in progress
};

// The list-mode loop of rect worlds (cornell-box: the F_BOXES | F_LIST kernel), rectangular.rs:27-57, :78-108,
// :129-159 for every rect, hittable/mod.rs:57-69 over them.  It walks the always list as runs of one wrapper
// chain and one kind (DevScene::lgroups): per chain the object-space ray, per run one specialised loop, so a rect
// costs no chain check and no type dispatch -- the scalar unit, which one CU's four SIMDs share, had become the
// limit of this loop (~35 SALU per rect against 17 VALU, profiles/r05/experiments).
// Fast path (wave-uniform, per chain): the division (k - o_k) / d_k is Markstein's correction from
// y_k = RN(1 / d_k) (rcp_rn_fast, exact in [2^-126, 2^126]; 3 VALU instead of the IEEE division's 11), the IEEE
// quotient whenever |d_k| is in [2^-60, 2^60] and |k - o_k| < 2^64 (|k| < 2^62 for every rect, DevScene::rect_fast;
// |o_k| < 2^62 per lane): then nothing over- or underflows unless |quotient| < 2^-42, where both are < TMIN and
// rejected alike (Markstein 1990; div_by_recip).  There t, the hit point's x, y are finite or +-inf, and the
// reference's tests `t >= TMIN`, `t <= best` and `!(x < a0 || x > a1)` are med3(v, lo, hi) == v (lo <= hi holds:
// TMIN <= best always, a0 <= a1 for every rect, DevScene::rect_fast): 3 med3, 3 subtractions, one max3 and one
// compare instead of 6 compares and 5 scalar ands.  A chain where any lane of the wave is outside that range runs the reference's IEEE
// division and compares (slow path).  The list is in DFS-key order, so a later rect wins a tie: accept t <= best
// (no key compare; bt starts at the reference's t_max = inf: a fast-path t is finite).  VERDICT r4 item 3.
template <int AXIS, bool FAST>
__device__ __forceinline__ void rect_list_test(const Ray& lr, V3 y, float4 q0, float k, uint32_t pi, float& bt,
                                               int32_t& bp) {
  const float o_k = AXIS == 0 ? lr.o.z : (AXIS == 1 ? lr.o.y : lr.o.x);
  const float d_k = AXIS == 0 ? lr.d.z : (AXIS == 1 ? lr.d.y : lr.d.x);
  const float y_k = AXIS == 0 ? y.z : (AXIS == 1 ? y.y : y.x);
  const float o_a = AXIS == 2 ? lr.o.y : lr.o.x, d_a = AXIS == 2 ? lr.d.y : lr.d.x;
  const float o_b = AXIS == 0 ? lr.o.y : lr.o.z, d_b = AXIS == 0 ? lr.d.y : lr.d.z;
  const float num = k - o_k;
  bool acc;
  if constexpr (FAST) {
    const float t = div_by_recip(num, d_k, y_k);
    const float x = o_a + t * d_a;
    const float yy = o_b + t * d_b;
    // the three tests as one: each med3 equals its value exactly when in range, so the largest |med3 - value| is 0 exactly
    // when all pass (t finite; x, y finite or +-inf, and +-inf lies outside the rect's finite bounds, rect_fast: inf, a
    // rejection as the reference's).  One compare, no scalar ands (+2 VALU, -2 SALU per rect: cornell-800 +1.5%, r05z)
    const float m1 = __builtin_amdgcn_fmed3f(t, TMIN, bt), m2 = __builtin_amdgcn_fmed3f(x, q0.x, q0.y);
    const float m3 = __builtin_amdgcn_fmed3f(yy, q0.z, q0.w);
    acc = fmaxf(fmaxf(fabsf(m1 - t), fabsf(m2 - x)), fabsf(m3 - yy)) == 0.0f;
    bt = acc ? t : bt;
    bp = acc ? (int32_t)pi : bp;
  } else {
    // the reference's own comparisons, rejections that a NaN passes (rectangular.rs:33-41): a ray in the
    // rect's plane (d_k = 0, k - o_k = 0: a Lambertian bounce whose direction lost its normal component) has
    // t = 0 / 0 and hits.  The reference's best is then NaN, under which every later rect whose own test passes
    // wins -- exactly as under best = +inf -- so bt keeps +inf (never NaN: the fast path's med3 needs an ordered
    // bound) and bp carries RECT_NAN_HIT; trace_rect_list hands the winner on with t = NaN.
    const float t = num / d_k;
    const float x = o_a + t * d_a;
    const float yy = o_b + t * d_b;
    const bool out = (x < q0.x) | (x > q0.y) | (yy < q0.z) | (yy > q0.w);
    acc = !(t < TMIN) & !(t > bt) & !out;
    const bool tnan = t != t;
    bt = acc ? (tnan ? INFINITY : t) : bt;
    bp = acc ? ((int32_t)pi | (tnan ? RECT_NAN_HIT : 0)) : bp;
  }
}

// one run of rects of one kind (AXIS) and chain: the whole 64-B record in one scalar load (s_load_dwordx16)
template <bool COUNT, int AXIS, bool FAST>
__device__ __forceinline__ void rect_list_run(const DevScene& S, uint32_t first, uint32_t count, const Ray& lr, V3 y,
                                              float& bt, int32_t& bp, uint32_t* cnt) {
  // the 5 dwords a test reads (a0, a1, b0, b1, k) as one s_load_dwordx8 per 64-B record (not the whole record as
  // s_load_dwordx16): both records of a trip fit the SGPRs at once, so their loads share one wait (cornell-800 +1.1%,
  // r05z2)
  typedef uint32_t u8v __attribute__((ext_vector_type(8)));
  const __attribute__((address_space(4))) u8v* P = (const __attribute__((address_space(4))) u8v*)(S.prims + first);
  auto one = [&](const u8v& rec, uint32_t k) {
    const float4 q0 = make_float4(__uint_as_float(rec[0]), __uint_as_float(rec[1]), __uint_as_float(rec[2]),
                                  __uint_as_float(rec[3]));
    rect_list_test<AXIS, FAST>(lr, y, q0, __uint_as_float(rec[4]), first + k, bt, bp);
    if (COUNT) { cnt[1]++; cnt[2 + PT_RECT_XY + AXIS]++; simd_tick(cnt, 10, 11); }
  };
  uint32_t k = 0;
  const __attribute__((address_space(4))) u8v* Pk = P;
  for (; k + 1u < count; k += 2u, Pk += 4) {  // two rects per trip (a Cuboid's runs are pairs)
    const u8v r0 = Pk[0], r1 = Pk[2];
    one(r0, k);
    one(r1, k + 1u);
  }
  if (k < count) {
    const u8v rl = Pk[0];
    one(rl, k);
  }
}

// a whole Cuboid (GK_BOX6): its xy, xz and yz pairs back to back, no run dispatch between them
template <bool COUNT, bool FAST>
__device__ __forceinline__ void rect_box6_run(const DevScene& S, uint32_t first, const Ray& lr, V3 y, float& bt,
                                              int32_t& bp, uint32_t* cnt) {
  rect_list_run<COUNT, 0, FAST>(S, first, 2u, lr, y, bt, bp, cnt);
  rect_list_run<COUNT, 1, FAST>(S, first + 2u, 2u, lr, y, bt, bp, cnt);
  rect_list_run<COUNT, 2, FAST>(S, first + 4u, 2u, lr, y, bt, bp, cnt);
}

template <bool COUNT>
__device__ __forceinline__ void trace_rect_list(const DevScene& S, const Ray& r, Best& best, uint32_t* cnt) {
  float bt = INFINITY;  // lib.rs:102 t_max
  int32_t bp = -1;
  uint32_t cur = 0xFFFFFFFFu;
  Ray lr = r;
  V3 y = mk(0.f, 0.f, 0.f);
  bool fast = false;
  for (uint32_t g = 0; g < S.n_lgroups; ++g) {
    const uint4 G = uload(reinterpret_cast<const uint4*>(S.lgroups + g));  // (first, count, instance, kind)
    if (G.z != cur) {  // wave-uniform
      cur = G.z;
      lr = r;
      if (cur) {  // a Cuboid's rotate_y + translate: both ops' loads at once, one wait (to_local's ops in order;
                  // cornell-800 +0.8%, r05z10)
        const DevInst* I = S.insts + cur;
        const uint32_t n = uload(&I->nops);
        const float4 op0 = uload(reinterpret_cast<const float4*>(I->op[0]));
        const float4 op1 = uload(reinterpret_cast<const float4*>(I->op[1]));
        auto apply = [&](const float4& op) {
          if (op_is(op.x, IO_TRANSLATE)) {
            lr.o = sub(lr.o, mk(op.y, op.z, op.w));
          } else {
            const float sn = op.y, c = op.z;
            lr.o = mk(c * lr.o.x - sn * lr.o.z, lr.o.y, sn * lr.o.x + c * lr.o.z);
            lr.d = mk(c * lr.d.x - sn * lr.d.z, lr.d.y, sn * lr.d.x + c * lr.d.z);
          }
        };
        if (n >= 1u) apply(op0);
        if (n >= 2u) apply(op1);
        for (uint32_t k = 2; k < n; ++k) apply(uload(reinterpret_cast<const float4*>(I->op[k])));
      }
      y = mk(rcp_rn_fast(lr.d.x), rcp_rn_fast(lr.d.y), rcp_rn_fast(lr.d.z));
      // the fast path's ranges (|d_k| in [2^-60, 2^60], |o_k| < 2^62), tested stricter on sums (a NaN or infinite
      // component makes its sum fail; a sum within the bound bounds each term): three compares instead of nine and
      // two scalar ands instead of eight (cornell-800 +1.9%, r05z7); a stricter test only sends more lanes to the
      // IEEE path
      const float dmin = fminf(fminf(fabsf(lr.d.x), fabsf(lr.d.y)), fabsf(lr.d.z));
      const float dsum = (fabsf(lr.d.x) + fabsf(lr.d.y)) + fabsf(lr.d.z);
      const float osum = (fabsf(lr.o.x) + fabsf(lr.o.y)) + fabsf(lr.o.z);
      const bool ok = (dmin >= 0x1p-60f) & (dsum <= 0x1p60f) & (osum < 0x1p62f);
      fast = S.rect_fast && __ballot(!ok) == 0;
    }
    if (fast) {
      if (G.w == GK_BOX6) rect_box6_run<COUNT, true>(S, G.x, lr, y, bt, bp, cnt);
      else if (G.w == PT_RECT_XY) rect_list_run<COUNT, 0, true>(S, G.x, G.y, lr, y, bt, bp, cnt);
      else if (G.w == PT_RECT_XZ) rect_list_run<COUNT, 1, true>(S, G.x, G.y, lr, y, bt, bp, cnt);
      else rect_list_run<COUNT, 2, true>(S, G.x, G.y, lr, y, bt, bp, cnt);
    } else {
      if (G.w == GK_BOX6) rect_box6_run<COUNT, false>(S, G.x, lr, y, bt, bp, cnt);
      else if (G.w == PT_RECT_XY) rect_list_run<COUNT, 0, false>(S, G.x, G.y, lr, y, bt, bp, cnt);
      else if (G.w == PT_RECT_XZ) rect_list_run<COUNT, 1, false>(S, G.x, G.y, lr, y, bt, bp, cnt);
      else rect_list_run<COUNT, 2, false>(S, G.x, G.y, lr, y, bt, bp, cnt);
    }
  }
  // an in-plane hit won (RECT_NAN_HIT; bp < 0 = no hit): the reference's t is NaN
  const bool nan_hit = bp >= 0 && (bp & RECT_NAN_HIT) != 0;
  best.t = nan_hit ? __builtin_nanf("") : bt;
  best.prim = nan_hit ? (bp & ~RECT_NAN_HIT) : bp;
}

// ---- far-origin rays (round 6; rtw_flatten.cpp's header)
// The BVH's sphere leaves are padded for origins within D0 of every BVH point.  From farther away (a path bouncing
// inside the r = 1000 ground sphere: ~5% of jumpy-balls' segments) the reference's f32 sphere test "hits" a sphere
// up to delta(D) outside it (its cancellation grows with D²), and its flat list finds such a hit wherever it lies.
// trace_begin tests the BVH box grown by delta(D) first -- almost every far ray misses it and skips the BVH -- and
// the rest (~5e-5 of jumpy-balls' segments) walk the tree here with every box grown by delta(D): a stack walk over
// the f32 node table (order never changes the answer: closest t, ties to the larger key) that descends into the
// nearest child hit, the lane's own LDS stack column as its stack (its main walk has not started), each hit leaf's
// primitives tested in turn.  A push past the column (never for a tree whose stack bound fits it) sends the lane
// through every BVH primitive.  Inlined into the main kernels, where the segment starts (profiles/r06/experiments:
// a far-path kernel that replayed the few paths needing it cost the same at 1080p but added its tail, one path's
// latency, to every frame: configs[0] -30%).
// The DevFar record, DEVFAR_BACK bytes before the prim table, re-derived at each use (the asm hides the pointer's
// provenance): otherwise the compiler hoists its ~20 kernel-uniform values into SGPRs held across the whole path
// loop, which spilled other SGPRs into VGPR lanes (v_readlane / v_writelane in the hot loop: jumpy-1080p -7%)
__device__ __forceinline__ const DevFar* far_record(const DevScene& S) {
  const char* p = reinterpret_cast<const char*>(S.prims);
  asm volatile("" : "+s"(p));
  return reinterpret_cast<const DevFar*>(p - DEVFAR_BACK);
}
// The walks' culling arithmetic (conservative, never the answer): the reciprocal of a direction component, kept
// finite, and the far limit of a box test, the best hit's t with slack
__device__ __forceinline__ float cull_inv(float d) {
  const float dd = fabsf(d) > 1e-20f ? d : copysignf(1e-20f, d);
  return __builtin_amdgcn_rcpf(dd);
}
__device__ __forceinline__ float cull_tmax(float t) { return __builtin_fmaf(t, 1.0e-5f, t) + 1.0e-5f; }
template <bool COUNT, uint32_t FEAT, int STACK, int BLK, bool C16, int NCAP>
__device__ void trace_far(const DevScene& S, const Ray& r, Best& b, float delta, uint16_t* stk16, int32_t* stk,
                          uint32_t* cnt, uint64_t seg, uint32_t* err, const float4* lnodes) {
  const DevFar* const FR = far_record(S);
  // the f32 node table: the workgroup's LDS copy in the LDS-node kernels, else global memory
  const char* const NB = NCAP > 0 ? reinterpret_cast<const char*>(lnodes)
                                  : reinterpret_cast<const char*>(S.prims) - uload(&FR->nodes_back);
  const uint32_t n_bvh = uload(&FR->n_bvh);
  const V3 inv = mk(cull_inv(r.d.x), cull_inv(r.d.y), cull_inv(r.d.z));
  const V3 ood = mk(r.o.x * inv.x, r.o.y * inv.y, r.o.z * inv.z);
  // every box grown by delta: its near plane delta |inv| earlier, its far plane delta |inv| later
  const V3 bn = mk(-ood.x - delta * fabsf(inv.x), -ood.y - delta * fabsf(inv.y), -ood.z - delta * fabsf(inv.z));
  const V3 bf = mk(-ood.x + delta * fabsf(inv.x), -ood.y + delta * fabsf(inv.y), -ood.z + delta * fabsf(inv.z));
  const uint32_t nx = inv.x < 0.f ? 16u : 0u, ny = (inv.y < 0.f ? 16u : 0u) + 32u, nz = (inv.z < 0.f ? 16u : 0u) + 64u;
  const uint32_t fx = nx ^ 16u, fy = ny ^ 16u, fz = nz ^ 16u;
  int32_t node = 0, sp = 0;
  bool over = false;
  for (uint32_t guard = 0;; ++guard) {
    if (node < 0) {
      if (sp == 0) break;
      --sp;
      node = C16 ? (int32_t)stk16[sp * BLK] : stk[sp * BLK];
    }
    if (guard >= (1u << 20)) {  // a corrupt tree (cycle): end the walk and report, as trace_run does
      *err = 1u;
      b.prim = -2;
      return;
    }
    if (COUNT) cnt[0]++;
    const uint32_t nb = (uint32_t)node << 7;  // sizeof(DevNode4)
    const float4 qnx = *reinterpret_cast<const float4*>(NB + (nb + nx)), qfx = *reinterpret_cast<const float4*>(NB + (nb + fx));
    const float4 qny = *reinterpret_cast<const float4*>(NB + (nb + ny)), qfy = *reinterpret_cast<const float4*>(NB + (nb + fy));
    const float4 qnz = *reinterpret_cast<const float4*>(NB + (nb + nz)), qfz = *reinterpret_cast<const float4*>(NB + (nb + fz));
    // 16-bit codes (0 = empty) or the 32-bit child words (0 = empty: the root is nobody's child)
    const uint4 cw = *reinterpret_cast<const uint4*>(NB + (nb + (C16 ? 112u : 96u)));
    const float tmax_c = cull_tmax(b.t);
    const float NX[4] = {qnx.x, qnx.y, qnx.z, qnx.w}, FX[4] = {qfx.x, qfx.y, qfx.z, qfx.w};
    const float NY[4] = {qny.x, qny.y, qny.z, qny.w}, FY[4] = {qfy.x, qfy.y, qfy.z, qfy.w};
    const float NZ[4] = {qnz.x, qnz.y, qnz.z, qnz.w}, FZ[4] = {qfz.x, qfz.y, qfz.z, qfz.w};
    const uint32_t W[4] = {cw.x, cw.y, cw.z, cw.w};
    uint32_t hits = 0;
    // the nearest internal child hit is walked next (the others pushed): the leaves met first shrink best t
    float tnear = INFINITY;
    int kn = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float tn = fmaxf(fmaxf(fmaxf(__builtin_fmaf(NX[k], inv.x, bn.x), __builtin_fmaf(NY[k], inv.y, bn.y)),
                                   __builtin_fmaf(NZ[k], inv.z, bn.z)), 0.0f);
      const float tf = fminf(fminf(fminf(__builtin_fmaf(FX[k], inv.x, bf.x), __builtin_fmaf(FY[k], inv.y, bf.y)),
                                   __builtin_fmaf(FZ[k], inv.z, bf.z)), tmax_c);
      const bool h = W[k] != 0u && tn <= tf;
      hits |= h ? 1u << k : 0u;
      const bool inner = C16 ? (W[k] & 0x8000u) == 0u : (int32_t)W[k] >= 0;
      const bool nearer = h && inner && tn < tnear;
      tnear = nearer ? tn : tnear;
      kn = nearer ? k : kn;
    }
    node = kn < 0 ? -1 : (int32_t)(kn == 0 ? W[0] : (kn == 1 ? W[1] : (kn == 2 ? W[2] : W[3])));
    hits &= kn < 0 ? hits : ~(1u << kn);
    while (hits) {
      const int k = __builtin_ctz(hits);
      hits &= hits - 1u;
      const uint32_t w = k == 0 ? W[0] : (k == 1 ? W[1] : (k == 2 ? W[2] : W[3]));
      if (C16 ? (w & 0x8000u) != 0u : (int32_t)w < 0) {  // a leaf: its primitives now
        const uint32_t v = C16 ? w & 0xFFFFu : ~w;
        const uint32_t first = C16 ? (v >> 2) & 0x1FFFu : v >> 3, n = C16 ? (v & 3u) + 1u : v & 7u;
        for (uint32_t q = 0; q < n; ++q) test_prim<COUNT, FEAT>(S, first + q, r, b, cnt, seg);
      } else if (sp < STACK) {
        if constexpr (C16) stk16[sp * BLK] = (uint16_t)w;
        else stk[sp * BLK] = (int32_t)w;
        ++sp;
      } else {
        over = true;  // the subtree is covered by the flat pass below
      }
    }
  }
  if (over)
    for (uint32_t pi = 0; pi < n_bvh; ++pi) test_prim<COUNT, FEAT>(S, pi, r, b, cnt, seg);
}

// Kernel variants that carry the far-origin path: BVH walks that may test spheres.  Not the mesh kernels (F_MESHES):
// a mesh world with spheres in its BVH (DevScene::far_check without bvh_tri) runs the generic kernel instead
// (pick_kernel), since even unexecuted the far code cost cow-1080p 0.6% and monument-4k 0.3% (r06)
constexpr bool far_kernel_feat(uint32_t feat) {
  return !(feat & F_LIST) && (feat & (F_SPHERE | F_MSPHERE | F_MEDIUM)) && feat != F_MESHES;
}
// C16: the kernel's LDS stack holds 16-bit entries (the LDS-node and S16 walks), else 32-bit ones (stk); trace_far
// borrows the lane's column.  A lane whose segment needs the far-origin walk takes it here, instead of the main walk.
// RING (the 1024-lane sphere kernel's start ring, path_kernel): `start` is what the lane's ring entry decided for this
// segment -- a primitive index (the segment's closest hit: the lane tests that primitive alone, so ts.b gets the same
// t from the same test, and takes no root) or -3 (undecided, and every later segment: the always list and the walk as
// ever); a start that the ring's make resolved to a miss never gets here (the make retires it).  One loop serves both,
// the index per lane, so a decided lane adds no instruction stream of its own.
template <bool COUNT, uint32_t FEAT, int STACK = 1, int BLK = BLOCK, bool C16 = false, int NCAP = 0, bool RING = false>
__device__ __forceinline__ void trace_begin(const DevScene& S, const Ray& r, TraceState& ts, uint32_t* cnt,
                                            uint64_t seg, uint16_t* stk16 = nullptr, int32_t* stk = nullptr,
                                            uint32_t* err = nullptr, const float4* lnodes = nullptr,
                                            int32_t start = -3) {
  ts.b = Best{INFINITY, 0u, -1, 0.0f, 0.0f};
  const bool decided = RING && start != -3;
  // list-mode worlds of rects only (the F_BOXES | F_LIST kernel)
  constexpr bool RECT_LIST = (FEAT & F_LIST) && (FEAT & F_RECT) && !(FEAT & (F_SPHERE | F_MSPHERE | F_TRI | F_MEDIUM));
  if constexpr (RECT_LIST) {
    trace_rect_list<COUNT>(S, r, ts.b, cnt);
  } else if (FEAT & F_INST) {
    // the always list is wave-uniform and in DFS order, so a wrapper chain's prims are adjacent
    // (a Cuboid's 6 sides): transform the ray once per chain instead of once per prim
    uint32_t cur = 0;
    Ray lr = r;
    // the always-tested prims are the last n_always of the prim table, in order (rtw_flatten.cpp appends them
    // after the BVH's): their indices need no load from S.always, so a prim's record loads do not wait on one
    // (cornell-800 +4.7%: 18 prims per segment; cow +1.5%, monument +0.6%; experiments a1)
    const uint32_t a0 = S.n_prims - S.n_always;
    for (uint32_t k = 0; k < S.n_always; ++k) {
      const uint32_t pi = a0 + k;
      const uint32_t inst = uload(&S.prims[pi].type_inst) >> 8;
      if (inst != cur) {
        lr = inst ? to_local<true>(S.insts + inst, r) : r;
        cur = inst;
      }
      test_prim<COUNT, FEAT, true, true>(S, pi, lr, ts.b, cnt, seg);
    }
  } else if constexpr (RING) {
    // (measured against a second form -- every lane the scalar always loop, then the lanes whose winner is a BVH
    // primitive one more test of their own -- this one loop was 1.6% faster: profiles/r08/experiments)
    const SphRcp rq = sph_rcp(r);
    const uint32_t n = decided ? 1u : S.n_always;
    for (uint32_t k = 0; __any(k < n); ++k) {
      if (k < n) {
        const uint32_t pi = decided ? (uint32_t)start : uload(S.always + k);
        test_prim<COUNT, FEAT, false, false>(S, pi, r, ts.b, cnt, seg, &rq);
      }
    }
  } else {
    constexpr bool SPH_ONLY = (FEAT & (F_RECT | F_TRI | F_MEDIUM | F_INST)) == 0 && (FEAT & (F_SPHERE | F_MSPHERE));
    SphRcp rq;
    if constexpr (SPH_ONLY) rq = sph_rcp(r);
    // (the loaded index here: the computed one made the sphere kernels 1.1% slower, experiments a1)
    for (uint32_t k = 0; k < S.n_always; ++k)
      test_prim<COUNT, FEAT, false, true>(S, uload(S.always + k), r, ts.b, cnt, seg, SPH_ONLY ? &rq : nullptr);
  }
  if constexpr ((FEAT & F_LIST) && !RECT_LIST) {  // an in-plane (NaN) winner: the reference's t is NaN
    const bool nan_hit = ts.b.prim >= 0 && (ts.b.prim & RECT_NAN_HIT) != 0;
    ts.b.t = nan_hit ? __builtin_nanf("") : ts.b.t;
    ts.b.prim = nan_hit ? (ts.b.prim & ~RECT_NAN_HIT) : ts.b.prim;
  }
  // far-origin rays (above): the BVH box grown by delta(D) over [0, best], then trace_far for the few that reach it;
  // neither takes the main walk
  bool walk = true;
#if defined(RTW_DIAG_FAR)  // timing diagnostic: 1 = no far check (pads only), 2 = far lanes skip the BVH, 3 = no far walk
                          // (the slab test's result unused: removed), 5 = the slab test kept, no far walk
  constexpr int DF = RTW_DIAG_FAR;
#else
  constexpr int DF = 0;
#endif
  constexpr bool FAR = DF != 1 && far_kernel_feat(FEAT);
  if constexpr (FAR) {
    if (S.far_check) {  // kernel-uniform
      const float4* const FR = reinterpret_cast<const float4*>(far_record(S));
      const float4 mid = uload(FR), half = uload(FR + 1);  // (mid, d2), (half, q)
      const float tx = fabsf(r.o.x - mid.x) + half.x;
      const float ty = fabsf(r.o.y - mid.y) + half.y;
      const float tz = fabsf(r.o.z - mid.z) + half.z;
      const float D2 = tx * tx + ty * ty + tz * tz;  // the farthest corner of the BVH box, squared
      const bool far = D2 > mid.w && !decided;  // (a decided start's origin is near: the host's condition for lists)
      if (__any(far)) {
        bool need = false;
        float delta = 0.0f;
        if (far && DF != 2) {
          const float4 lo = uload(FR + 2), hi = uload(FR + 3), e = uload(FR + 4);  // (lo, q0), (hi, s), (s0, l, l0)
          // D from v_sqrt_f32 (1 ulp) rounded up; delta grows with D
          const float D = __builtin_amdgcn_sqrtf(D2) * 1.000001f;
          delta = fminf(half.w * D2 + lo.w, hi.w * D + e.x) + (e.y * D + e.z);
          // the BVH box grown by delta, centred: |p - mid| <= half + delta per axis, over [0, best].  Raw reciprocals:
          // a zero direction component gives +-inf planes (the axis unconstrained, or a miss), and a NaN (0 * inf: the
          // origin exactly on a grown plane, the ray in it) drops out of fminf / fmaxf as a miss -- correct, since the
          // spurious-hit region lies strictly inside the grown box (delta has 1% to spare)
          const float ix = __builtin_amdgcn_rcpf(r.d.x), iy = __builtin_amdgcn_rcpf(r.d.y), iz = __builtin_amdgcn_rcpf(r.d.z);
          const float ox = r.o.x - mid.x, oy = r.o.y - mid.y, oz = r.o.z - mid.z;
          const float hx = half.x + delta, hy = half.y + delta, hz = half.z + delta;
          const float ax = (-hx - ox) * ix, bx = (hx - ox) * ix, ay = (-hy - oy) * iy, by = (hy - oy) * iy;
          const float az = (-hz - oz) * iz, bz = (hz - oz) * iz;
          const float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), 0.0f));
          const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)),
                                 fminf(fmaxf(az, bz), cull_tmax(ts.b.t)));
          need = tn <= tf;
        }
        walk = !far;
        if (DF == 5) asm volatile("" ::"v"((uint32_t)need));  // timing diagnostic: the test kept, no far walk
        if (DF != 3 && DF != 5 && __builtin_expect(__any(need), 0))
          if (need) trace_far<COUNT, FEAT, STACK, BLK, C16, NCAP>(S, r, ts.b, delta, stk16, stk, cnt, seg, err, lnodes);
      }
    }
  }
  // the root (or none) made opaque here: hoisted out of the path loop, the compiler kept it in a VGPR across the
  // whole loop and spilled it.  Triangle kernels (the mesh walk): as a scalar, since the 7-wave walk spilled even
  // the opaque VGPR copy to scratch (one reload per segment; s1)
  int32_t root = S.n_nodes ? 0 : -1;
  if constexpr ((FEAT & F_TRI) != 0) {
    root = __builtin_amdgcn_readfirstlane(root);
    asm volatile("" : "+s"(root));
  } else {
    asm volatile("" : "+v"(root));
  }
  ts.node = (walk && !decided) ? root : -1;
  ts.pend = 0;
  ts.sp = 0;
  ts.on = true;
}

// while-while walk of the 4-wide BVH with postponed leaves (Aila & Laine 2009): phase 1 visits
// internal nodes (nearest hit child next, the other hit children pushed); a lane that reaches a
// leaf parks it (one slot; further leaves go on the stack) and keeps walking speculatively until
// every lane of the wave holds a leaf or has run dry; phase 2 tests all parked leaves together.
// NCAP > 0: the whole node table is in the workgroup's LDS (`lnodes`, copied at kernel start), so
// the 7 node loads of a visit are ds_read_b128s instead of vector-memory loads (TA/TD were 89/98%
// busy on jumpy-balls with the nodes in L1/L2).
//
// NCAP > 0 also switches to the sorted-push walk over 16-bit stack entries (`stk16`, rows of BLK
// halfwords) of the nodes' 16-bit child codes (DevNode4::code: internal = node4 index, leaf =
// 0x8000 | first << 2 | (count - 1)), and a visit
//   * keys every hit child as (its entry distance's float bits, top 16) | code, a miss as 0,
//   * sorts the 4 keys descending (10 min/max) and writes all four codes to stack rows sp..sp+3
//     (one address, constant offsets; rows past the new top are scratch: Flat::stack_need4),
//   * walks into the nearest hit child (the smallest non-zero key) and keeps the others pushed,
//     farthest deepest; a nearest leaf is parked, or stays pushed if the parking slot is taken.
// It replaces the per-child nearest / push bookkeeping of the 32-bit walk (a visit: 97 -> 91 VALU,
// 44 of them the slab tests) and halves the stack's LDS.
// Which nodes are visited in which order never changes the answer (closest hit, ties to the
// larger key, over every leaf not culled).
// HN: the walk reads the half-precision node table (DevNode4h: 4 loads / 64 B per visit instead of 7 / 112 B)
#ifndef RTW_MESH_ROOT
#define RTW_MESH_ROOT 5  // node4s of the S16 mesh walk's LDS copy of the tree top (trace_run ROOT; 0 = none, 1 = root)
#endif
#ifndef REGEN_RING
#define REGEN_RING 2  // regen_min of the kernels with the start ring
#endif
#ifndef REGEN_RING_LDSN
#define REGEN_RING_LDSN 8  // ... of the 1024-lane sphere kernel with it (jumpy-1080p: flat from 1 to 16, 8-12 best by 0.2%)
#endif
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ half2_t as_h2(uint32_t u) { return __builtin_bit_cast(half2_t, u); }

// S16: the global-node walk keeps 16-bit stack entries (the nodes' 16-bit codes, sign-extended: leaves < 0)
// in the uint16 column `stk16`, half the LDS of the 32-bit stack (RTW_MESH_S16: more workgroups per CU)
//
// ANY (occluded_kernel, rtw_occluded_kernel.hpp): an any-hit walk to the caller's bound `tcap` (>= TMIN, not NaN; a
// smaller bound takes no walk at all).  The answer asked for is `best.prim >= 0 && !(best.t > tcap)` of the closest
// hit, and every accepted candidate has t >= the closest t, so (1) a lane whose best satisfies it after a leaf phase
// is done -- its stack is dropped -- and (2) the slab tests cull at min(best t, tcap) (RTW_OCCLUDED_CULL; DESIGN.md
// §2: a box that holds a hit at t* <= tcap passes under any bound >= t*, and min(best, tcap) >= t*).  Best itself
// stays unseeded: the accept's tie rule would make a seeded bound exclusive for the leaf with key 0.
#ifndef RTW_OCCLUDED_CULL
#define RTW_OCCLUDED_CULL 1  // 0 = early retirement alone (the ablation of DESIGN.md §4)
#endif
template <bool COUNT, int STACK, bool SPILL, uint32_t FEAT, int BLK, int NCAP, bool HN = false, bool S16 = false,
          bool ANY = false>
__device__ void trace_run(const DevScene& S, const Ray& r, TraceState& ts, int32_t* stk, int32_t* spill,
                          uint32_t spill_lanes, uint32_t* cnt, uint32_t quota, uint32_t leaf_thr, uint64_t seg,
                          uint32_t* err, uint64_t* tph, const float4* lnodes, uint16_t* stk16,
                          float tcap = INFINITY) {
  // the slab tests' far limit: the best hit's t, in an any-hit walk no farther than the caller's bound
  auto cull_bound = [&]() { return cull_tmax((ANY && RTW_OCCLUDED_CULL) ? fminf(ts.b.t, tcap) : ts.b.t); };
  constexpr bool K16 = NCAP > 0;
  constexpr bool CODES = K16 || HN || S16;  // leaves are 16-bit codes (the 32-bit walk keeps them sign-extended)
  constexpr bool SPH_ONLY = (FEAT & (F_RECT | F_TRI | F_MEDIUM | F_INST)) == 0 && (FEAT & (F_SPHERE | F_MSPHERE));
  SphRcp rq;  // once per call: the sphere roots' divisor and its reciprocal
  if constexpr (SPH_ONLY) rq = sph_rcp(r);
  // triangle-only BVH (DevScene::bvh_tri): the leaves' common object-space ray, once per call
  Ray tri_ray = r;
  if constexpr ((FEAT & F_TRI) != 0) {
    if (S.bvh_tri && (FEAT & F_INST) && S.tri_inst) {
      if (S.tri_inst == S.uni_inst) tri_ray.o = sub(r.o, mk(S.uni_off[0], S.uni_off[1], S.uni_off[2]));
      else tri_ray = to_local<true>(S.insts + S.tri_inst, r);
    }
  }
  // COUNT: tph[0] += wave-cycles in the node loop (phase 1), tph[1] += in the leaf tests (phase 2)
  uint64_t tm = COUNT ? __builtin_amdgcn_s_memtime() : 0;
  // Waves walking the tree issue before waves shading or regenerating (the path kernel drops the
  // priority again when trace_run returns).  MI355X A/B (profiles/r02/experiments, s1/s2): jumpy
  // +1.7%, cow +1.6%, monument +0.7%; shading first, node-load issue first or graded levels were
  // slower or equal.
  // The LDS-node kernel (NCAP > 0, node loads from LDS) is 0.6% faster without it (experiments, p2).
  if constexpr (NCAP == 0) __builtin_amdgcn_s_setprio(2);
  auto tick = [&](int k) {
    if (COUNT) {
      const uint64_t t = __builtin_amdgcn_s_memtime();
      tph[k] += t - tm;
      tm = t;
    }
  };
  const V3 inv = mk(cull_inv(r.d.x), cull_inv(r.d.y), cull_inv(r.d.z));
  const V3 ood = mk(r.o.x * inv.x, r.o.y * inv.y, r.o.z * inv.z);
  // near / far plane byte offsets inside DevNode4 by the ray's direction signs (32-bit offsets
  // from the uniform table base: the loads take the SGPR-base + VGPR-offset form)
  const uint32_t nx = inv.x < 0.f ? 16u : 0u, ny = (inv.y < 0.f ? 16u : 0u) + 32u, nz = (inv.z < 0.f ? 16u : 0u) + 64u;
  const uint32_t fx = nx ^ 16u, fy = ny ^ 16u, fz = nz ^ 16u;
  const char* const NB = NCAP > 0 ? reinterpret_cast<const char*>(lnodes)
                                  : (HN ? reinterpret_cast<const char*>(S.hnodes) : reinterpret_cast<const char*>(S.nodes));
  // ROOT (the S16 half-node mesh walk): lanes at the root or one of its children (breadth-first ids 0..4) visit it
  // from the workgroup's LDS copy of those five node4s (lnodes) before the loop, twice, so a segment's first two
  // visits cost no vector-memory loads (the mesh kernels are bound on the vector-memory data path, TD: ~2 of
  // monument's 5.6 visits per ray).  monument-4k +0.7%, cow-1080p +0.5-0.7% (profiles/r06/experiments rt5); the
  // same in the loop itself (t1: the tree's top from LDS at every visit) lost 6%: a visit whose lanes straddle the
  // table's edge runs both load paths, and the branch breaks up the loop's load clause.  17 node4s, three levels: -3.6%.
  constexpr bool ROOT = HN && S16 && NCAP == 0 && RTW_MESH_ROOT > 0;
  constexpr int32_t NROOT = RTW_MESH_ROOT;  // node4s in the LDS copy: 1 = the root, 5 = the root and its children
#pragma unroll
  for (int lv = 0; lv < (ROOT ? (NROOT > 1 ? 2 : 1) : 0); ++lv) {
    if (__any(ts.node >= 0 && ts.node < NROOT)) {
      if (ts.node >= 0 && ts.node < NROOT) {
        const char* const TB = reinterpret_cast<const char*>(lnodes) + (uint32_t)ts.node * 112u;
        const uint4 px = *reinterpret_cast<const uint4*>(TB + nx);
        const uint4 py = *reinterpret_cast<const uint4*>(TB + ny);
        const uint4 pz = *reinterpret_cast<const uint4*>(TB + nz);
        const uint4 cq = *reinterpret_cast<const uint4*>(TB + 96u);
        const half2_t oxy = as_h2(cq.z), oz = as_h2(cq.w);
        const V3 bs = mk(__builtin_fmaf((float)oxy.x, inv.x, -ood.x), __builtin_fmaf((float)oxy.y, inv.y, -ood.y),
                         __builtin_fmaf((float)oz.x, inv.z, -ood.z));
        const uint32_t PQ[3][4] = {{px.x, px.y, px.z, px.w}, {py.x, py.y, py.z, py.w}, {pz.x, pz.y, pz.z, pz.w}};
        float NA[3][4], FA[3][4];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const half2_t n01 = as_h2(PQ[q][0]), n23 = as_h2(PQ[q][1]), f01 = as_h2(PQ[q][2]), f23 = as_h2(PQ[q][3]);
          NA[q][0] = (float)n01.x; NA[q][1] = (float)n01.y; NA[q][2] = (float)n23.x; NA[q][3] = (float)n23.y;
          FA[q][0] = (float)f01.x; FA[q][1] = (float)f01.y; FA[q][2] = (float)f23.x; FA[q][3] = (float)f23.y;
        }
        const int32_t CW[4] = {(int32_t)(int16_t)(cq.x & 0xFFFFu), (int32_t)cq.x >> 16, (int32_t)(int16_t)(cq.y & 0xFFFFu),
                               (int32_t)cq.y >> 16};
        if (COUNT) {
          cnt[0]++;
          cnt[14] += (CW[0] != 0) + (CW[1] != 0) + (CW[2] != 0) + (CW[3] != 0);
        }
        const float tmax_c = cull_bound();
        int32_t next = -1, bk = -1;
        float best = INFINITY;
        bool hit[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // conservative slab test (culling only), as in the loop below
          const float a0 = __builtin_fmaf(NA[0][k], inv.x, bs.x), b0 = __builtin_fmaf(NA[1][k], inv.y, bs.y);
          const float c0 = __builtin_fmaf(NA[2][k], inv.z, bs.z);
          const float d0 = __builtin_fmaf(FA[0][k], inv.x, bs.x), e0 = __builtin_fmaf(FA[1][k], inv.y, bs.y);
          const float f0 = __builtin_fmaf(FA[2][k], inv.z, bs.z);
          const float tn = fmaxf(fmaxf(fmaxf(a0, b0), c0), 0.0f);
          hit[k] = tn <= fminf(fminf(fminf(d0, e0), f0), tmax_c);
          const bool in = hit[k] & (CW[k] >= 0) & (tn < best);
          best = in ? tn : best;
          bk = in ? k : bk;
          next = in ? CW[k] : next;
        }
        int32_t pend = ts.pend, sp = ts.sp;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool leaf_take = hit[k] & (CW[k] < 0) & (pend == 0);
          pend = leaf_take ? CW[k] : pend;
          const bool pk = hit[k] & (k != bk) & !leaf_take;
          stk16[sp * BLK] = (uint16_t)CW[k];
          sp += pk ? 1 : 0;
        }
        ts.pend = pend;
        ts.sp = sp;
        ts.node = next;
      }
    }
  }
  // every wave must drain: a corrupt tree (a cycle) ends the walk instead of hanging the GPU, and
  // sets the device's host-mapped error word (RenderArgs::err), which the host turns into RTW_EINVAL
  // at the next render call, rtw_render_status, rtw_path_kernel_times or a stats read
  constexpr uint32_t GUARD = 1u << 20;
  uint32_t guard = 0;
  for (; guard < GUARD; ++guard) {
    uint32_t g2 = 0;
    for (; g2 < GUARD; ++g2) {
      if constexpr (K16) {  // refill: pop a code (internal node, or a leaf if the parking slot is free)
        const bool can = ts.node < 0 && ts.sp > 0;
        const int32_t top = can ? (int32_t)stk16[(ts.sp - 1) * BLK] : 0;
        const bool leaf = (top & 0x8000) != 0;
        const bool popn = can && !leaf;
        const bool popl = can && leaf && ts.pend == 0;
        ts.node = popn ? top : ts.node;
        ts.pend = popl ? top : ts.pend;
        ts.sp -= (popn || popl) ? 1 : 0;
      } else {  // refill from the stack: an internal node, or a parked leaf if the slot is free
        const bool can = ts.node < 0 && ts.sp > 0;
        int32_t top = 0;
        if (can) {
          const int32_t i = ts.sp - 1;
          if constexpr (S16) {
            top = (int32_t)(int16_t)stk16[i * BLK];
          } else {
            top = stk[(SPILL ? min(i, STACK) : i) * BLK];
            if (SPILL && i >= STACK) top = spill[(size_t)(i - STACK) * spill_lanes];  // rare
          }
        }
        const bool popn = can && top >= 0;
        const bool popl = can && top < 0 && ts.pend == 0;
        ts.node = popn ? top : ts.node;
        ts.pend = popl ? top : ts.pend;
        ts.sp -= (popn || popl) ? 1 : 0;
      }
#ifdef RTW_LANE_DIAG
      if (COUNT) {  // lane states per node-loop iteration (diagnostic build): all, descending, parked, done
        const uint64_t bd = __ballot(ts.node >= 0), bp = __ballot(ts.node < 0 && ts.pend != 0);
        const uint64_t bn = __ballot(ts.node < 0 && ts.pend == 0 && ts.sp == 0);
        tph[3] += 64;  // per lane (the wave-uniform values are added by every lane: ratios are unaffected)
        tph[4] += (uint64_t)__popcll(bd);
        tph[5] += (uint64_t)__popcll(bp);
        tph[6] += (uint64_t)__popcll(bn);
      }
#endif
      if (!__any(ts.node >= 0 && ts.pend == 0)) break;
      // enough lanes hold a postponed leaf with nothing left to descend: test the leaves now instead of
      // waiting until no lane can descend (Aila & Laine's rule).  leaf_thr = 3/16 of the wave's lanes
      // (knob RTW_LEAF16), measured on MI355X against 1..16/16: monument +8%, cow +0.6%, jumpy -0.4%
      if ((uint32_t)__popcll(__ballot(ts.node < 0 && ts.pend != 0)) >= leaf_thr) break;
#ifdef RTW_UNI_DIAG
      if (COUNT) {  // diagnostic build: wave-level visits whose visiting lanes share the node (and octant)
        const uint64_t vis = __ballot(ts.node >= 0);
        const int src = (int)__ffsll((long long)vis) - 1;
        const int32_t n0 = __shfl(ts.node, src, 64);
        const uint32_t oct = nx | ny | nz, o0 = (uint32_t)__shfl((int)oct, src, 64);
        const bool un = __ballot(ts.node >= 0 && ts.node != n0) == 0;
        const bool uo = __ballot(ts.node >= 0 && (ts.node != n0 || oct != o0)) == 0;
        tph[3] += 1;
        tph[4] += uo ? 1 : 0;
        tph[5] += un ? 1 : 0;
        tph[6] += (uint64_t)__popcll(vis);
      }
#endif
      if (ts.node >= 0) {
        float NX[4], FX[4], NY[4], FY[4], NZ[4], FZ[4];
        int32_t CW[4];
        V3 bs;  // plane t = plane * inv + bs per axis
        if constexpr (HN) {
          // DevNode4h: per axis ONE 16-B load at offset 0 / 16 by direction sign = (near x4, far x4) as f16
          // offsets; then codes + origin.  t = off * inv + (origin * inv - o * inv): every product and
          // sum a v_fma_mix_f32 on the f16 halves.  The f16 boxes contain the f32 ones (outward rounding).
          const uint32_t nb = (uint32_t)ts.node * 112u;  // sizeof(DevNode4h)
          const uint4 px = *reinterpret_cast<const uint4*>(NB + (nb + nx));
          const uint4 py = *reinterpret_cast<const uint4*>(NB + (nb + ny));
          const uint4 pz = *reinterpret_cast<const uint4*>(NB + (nb + nz));
          const uint4 cq = *reinterpret_cast<const uint4*>(NB + (nb + 96u));
          const half2_t oxy = as_h2(cq.z), oz = as_h2(cq.w);
          bs = mk(__builtin_fmaf((float)oxy.x, inv.x, -ood.x), __builtin_fmaf((float)oxy.y, inv.y, -ood.y),
                  __builtin_fmaf((float)oz.x, inv.z, -ood.z));
          const uint32_t P[3][4] = {{px.x, px.y, px.z, px.w}, {py.x, py.y, py.z, py.w}, {pz.x, pz.y, pz.z, pz.w}};
          float* const NA[3] = {NX, NY, NZ};
          float* const FA[3] = {FX, FY, FZ};
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            const half2_t n01 = as_h2(P[a][0]), n23 = as_h2(P[a][1]), f01 = as_h2(P[a][2]), f23 = as_h2(P[a][3]);
            NA[a][0] = (float)n01.x; NA[a][1] = (float)n01.y; NA[a][2] = (float)n23.x; NA[a][3] = (float)n23.y;
            FA[a][0] = (float)f01.x; FA[a][1] = (float)f01.y; FA[a][2] = (float)f23.x; FA[a][3] = (float)f23.y;
          }
          if constexpr (K16) {  // the codes as they are
            CW[0] = (int32_t)(cq.x & 0xFFFFu); CW[1] = (int32_t)(cq.x >> 16);
            CW[2] = (int32_t)(cq.y & 0xFFFFu); CW[3] = (int32_t)(cq.y >> 16);
          } else {  // sign-extended: internal >= 0, leaf < 0, as the 32-bit walk's child words
            CW[0] = (int32_t)(int16_t)(cq.x & 0xFFFFu); CW[1] = (int32_t)cq.x >> 16;
            CW[2] = (int32_t)(int16_t)(cq.y & 0xFFFFu); CW[3] = (int32_t)cq.y >> 16;
          }
        } else {
          const uint32_t nb = (uint32_t)ts.node << 7;  // sizeof(DevNode4); n_nodes < 2^25 (flatten)
          constexpr uint32_t CWO = (K16 || S16) ? 112u : 96u;  // child codes (K16, S16) or child words
          const float4 qnx = *reinterpret_cast<const float4*>(NB + (nb + nx));
          const float4 qfx = *reinterpret_cast<const float4*>(NB + (nb + fx));
          const float4 qny = *reinterpret_cast<const float4*>(NB + (nb + ny));
          const float4 qfy = *reinterpret_cast<const float4*>(NB + (nb + fy));
          const float4 qnz = *reinterpret_cast<const float4*>(NB + (nb + nz));
          const float4 qfz = *reinterpret_cast<const float4*>(NB + (nb + fz));
          const int4 cw = *reinterpret_cast<const int4*>(NB + (nb + CWO));
          bs = neg(ood);
          NX[0] = qnx.x; NX[1] = qnx.y; NX[2] = qnx.z; NX[3] = qnx.w; FX[0] = qfx.x; FX[1] = qfx.y; FX[2] = qfx.z; FX[3] = qfx.w;
          NY[0] = qny.x; NY[1] = qny.y; NY[2] = qny.z; NY[3] = qny.w; FY[0] = qfy.x; FY[1] = qfy.y; FY[2] = qfy.z; FY[3] = qfy.w;
          NZ[0] = qnz.x; NZ[1] = qnz.y; NZ[2] = qnz.z; NZ[3] = qnz.w; FZ[0] = qfz.x; FZ[1] = qfz.y; FZ[2] = qfz.z; FZ[3] = qfz.w;
          if constexpr (S16 && !K16) {  // 16-bit codes, sign-extended: internal >= 0, leaf < 0
            CW[0] = (int32_t)(int16_t)cw.x; CW[1] = (int32_t)(int16_t)cw.y;
            CW[2] = (int32_t)(int16_t)cw.z; CW[3] = (int32_t)(int16_t)cw.w;
          } else {
            CW[0] = cw.x; CW[1] = cw.y; CW[2] = cw.z; CW[3] = cw.w;
          }
        }
        if (COUNT) {
          cnt[0]++;
          simd_tick(cnt, 8, 9);
          cnt[14] += (CW[0] != 0) + (CW[1] != 0) + (CW[2] != 0) + (CW[3] != 0);  // child word 0 = empty slot
        }
        const float tmax_c = cull_bound();
        float tn[4];
        bool hit[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // conservative slab test (culling only)
          const float a = __builtin_fmaf(NX[k], inv.x, bs.x), b = __builtin_fmaf(NY[k], inv.y, bs.y);
          const float c = __builtin_fmaf(NZ[k], inv.z, bs.z);
          const float d = __builtin_fmaf(FX[k], inv.x, bs.x), e = __builtin_fmaf(FY[k], inv.y, bs.y);
          const float f = __builtin_fmaf(FZ[k], inv.z, bs.z);
          tn[k] = fmaxf(fmaxf(fmaxf(a, b), c), 0.0f);
          hit[k] = tn[k] <= fminf(fminf(fminf(d, e), f), tmax_c);
        }
        if constexpr (K16) {
          // pin the child codes in registers: otherwise the compiler sinks each child's LDS read under
          // its `hit` branch (4 dependent read round trips per visit)
          int32_t cwv[4] = {CW[0], CW[1], CW[2], CW[3]};
          asm volatile("" : "+v"(cwv[0]), "+v"(cwv[1]), "+v"(cwv[2]), "+v"(cwv[3]));
          uint32_t key[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) key[k] = hit[k] ? ((__float_as_uint(tn[k]) & 0xFFFF0000u) | (uint32_t)cwv[k]) : 0u;
          const uint32_t a0 = max(key[0], key[1]), b0 = min(key[0], key[1]);
          const uint32_t c0 = max(key[2], key[3]), d0 = min(key[2], key[3]);
          const uint32_t s0 = max(a0, c0), x0 = min(a0, c0), y0 = max(b0, d0), s3 = min(b0, d0);
          const uint32_t s1 = max(x0, y0), s2 = min(x0, y0);
          uint16_t* w = stk16 + ts.sp * BLK;  // rows sp .. sp + 3 (ds_write_b16 stores the code bits)
          w[0] = (uint16_t)s0;
          w[BLK] = (uint16_t)s1;
          w[2 * BLK] = (uint16_t)s2;
          w[3 * BLK] = (uint16_t)s3;
          const bool m1 = s1 != 0u, m2 = s2 != 0u, m3 = s3 != 0u;
          const uint32_t near = m3 ? s3 : (m2 ? s2 : (m1 ? s1 : s0));
          const int32_t code = (int32_t)(near & 0xFFFFu);
          const bool any = s0 != 0u, leaf = (code & 0x8000) != 0;
          const bool park = any && leaf && ts.pend == 0;
          // pushed: the hits but the nearest (h - 1), + the nearest leaf if it cannot be parked
          ts.sp += (int32_t)m1 + (int32_t)m2 + (int32_t)m3 + ((any && leaf && !park) ? 1 : 0);
          ts.pend = park ? code : ts.pend;
          ts.node = (any && !leaf) ? code : -1;
          continue;
        }
        // nearest hit internal child -> next node; the other hit children -> stack / parked slot
        int32_t next = -1;
        float best = INFINITY;
        int bk = -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool in = hit[k] & (CW[k] >= 0) & (tn[k] < best);  // bitwise: no branches
          best = in ? tn[k] : best;
          bk = in ? k : bk;
          next = in ? CW[k] : next;
        }
        int32_t pend = ts.pend;
        uint32_t push = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool leaf_take = hit[k] & (CW[k] < 0) & (pend == 0);
          pend = leaf_take ? CW[k] : pend;
          push |= (hit[k] & (k != bk) & !leaf_take) ? (1u << k) : 0u;
        }
        ts.pend = pend;
        int32_t sp = ts.sp;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool pk = (push >> k) & 1u;
          // branch-free: a child that is not pushed is written where the next push (or nothing)
          // lands, i.e. at or above the final top, never below it.  Rows 0..STACK exist; with
          // SPILL, row STACK is scratch and entries from STACK up live in HBM (sp < stack_need).
          if constexpr (S16) {
            stk16[sp * BLK] = (uint16_t)CW[k];
          } else {
            stk[(SPILL ? min(sp, STACK) : sp) * BLK] = CW[k];
            if (SPILL && pk && sp >= STACK) spill[(size_t)(sp - STACK) * spill_lanes] = CW[k];  // rare
          }
          sp += pk ? 1 : 0;
        }
        ts.sp = sp;
        ts.node = next;
      }
    }
    if (g2 == GUARD) break;
    tick(0);
    if (ts.pend != 0) {  // phase 2
      const uint32_t v = CODES ? (uint32_t)ts.pend & 0xFFFFu : ~(uint32_t)ts.pend;
      const int32_t first = CODES ? (int32_t)((v >> 2) & 0x1FFFu) : (int32_t)(v >> 3);
      const int32_t n = CODES ? (int32_t)(v & 3u) + 1 : (int32_t)(v & 7u);
      if ((FEAT & F_TRI) && S.bvh_tri) {  // kernel-uniform: every leaf is a triangle of one wrapper chain
        for (int32_t k = 0; k < n; ++k) test_tri_leaf<COUNT>(S, (uint32_t)(first + k), tri_ray, ts.b, cnt);
      } else {
        for (int32_t k = 0; k < n; ++k)
          test_prim<COUNT, FEAT>(S, (uint32_t)(first + k), r, ts.b, cnt, seg, SPH_ONLY ? &rq : nullptr);
      }
      ts.pend = 0;
    }
    tick(1);
    if constexpr (ANY) {  // something within the bound: the lane has its answer
      const bool occ = ts.b.prim >= 0 && !(ts.b.t > tcap);
      ts.node = occ ? -1 : ts.node;
      ts.sp = occ ? 0 : ts.sp;
    }
    const uint64_t done = __ballot(ts.node < 0 && ts.sp == 0);
    if (done == __ballot(1) || (uint32_t)__popcll(done) >= quota) return;
  }
  *err = 1u;  // a guard tripped: end this traversal (miss) and report (a vector store to host memory)
  ts.b.prim = -2;  // the path kernel drains the grid (see its miss branch)
  ts.node = -1;
  ts.sp = 0;
  ts.pend = 0;
}

}  // namespace dev
}  // namespace rtw
