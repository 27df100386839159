// rtw_path_kernel.hpp — the persistent path kernel (Raytracer::render / sample_pixel / sample_ray, lib.rs:57-117):
// PathState, the path starts (StartArgs, start_path and its two halves start_make / start_take for the start ring),
// KernelCfg, a variant's one compile-time configuration with everything derived from it, and
// path_kernel<COUNT, KernelCfg K> itself.  Structure: rtw_kernel.hip's header and DESIGN.md §4.
#pragma once
#include "rtw_dev_shade.hpp"
#include "rtw_dev_trace.hpp"

namespace rtw {
namespace dev {

// ---- the persistent path kernel
//
// Work unit = one path (pixel, sample).  Path id p (within a pass) = (slot*spp + s)*64 + l:
// slot = tile slot, s = sample, l = lane-in-tile, so the 64 paths a wave draws together
// are one sample of one 8x8 tile (coherent camera rays).  Waves are persistent: whenever
// lanes finish a path, the wave hands them new ids from a per-wave pool (ballot + mbcnt
// prefix), refilled from a global counter BATCH ids at a time, so lanes stay busy and the
// grid drains with a one-path tail.  Each finished path writes L to the ordered sample
// buffer (path-major RGB, 12 B per path in HBM); reduce_kernel then sums each pixel's samples in
// sample order — exactly lib.rs:83-87's `pixel_color += sample_ray(..)` sequence.
// Path ids a wave takes per returning atomic on the global queue word (path_kernel SHARD: eight).  Every wave of
// the grid hits that word: at 256 ids per atomic, short-path scenes spent most of their time behind it
// (MI355X, RTW_BATCH sweep: cow-1080p 19.0k -> 30.1k Mrays/s, monument-4k 12.8k -> 17.0k, jumpy-1080p
// 19.4k -> 20.4k at 2048); the tail this leaves is one batch per wave (~0.1 ms).  Knob RTW_BATCH.
constexpr uint32_t BATCH = 2048;

struct PathState {
  Ray ray;
  V3 T;
  uint64_t rng;
  uint32_t pid;  // path id within the pass (a pass holds at most 2^32 paths, max_pass_paths)
  uint32_t depth;
};

// floor(n / d) for 32-bit n and d >= 2 from M = UINT64_MAX / d + 1 (Lemire, Kaser & Kurz 2019,
// "Faster remainder by direct computation"): hi64(M * n) in two 32-bit multiplies instead of the
// ~25-instruction runtime u32 division; checked exhaustively for 12 divisors over every n and for
// 1e8 random pairs on the host.
__device__ __forceinline__ uint32_t fastdiv(uint32_t n, uint64_t M) {
  const uint64_t t = (uint64_t)(uint32_t)(M >> 32) * n + __umulhi((uint32_t)M, n);
  return (uint32_t)(t >> 32);
}

// readfirstlane of a 64-bit value.  The builtin returns a signed int: each half must go through
// uint32_t before widening, or a low half >= 2^31 sign-extends over the high half (path ids of a
// pass above 2^31 — monument-4k's 2^32-path passes — became huge and wrote outside the buffer).
__device__ __forceinline__ uint64_t rfl64(uint64_t x) {
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32));
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
  return ((uint64_t)hi << 32) | lo;
}

// start_path's kernel-uniform operands (camera, frame and tile geometry, seeds): copied into LDS once per
// workgroup and re-read at every regeneration, instead of living in SGPRs across the whole path loop,
// where the list-mode and sphere kernels had to spill them into VGPR lanes (every reload a v_readlane).
struct StartArgs {
  DevCamera cam;
  float fw1, fh1, rw1, rh1, time_span;
  uint32_t w, h, spp, max_depth, tiles_x, slot_base, tile_first, tile_stride;
  uint64_t spp_magic, tiles_x_magic, seed_hash;
  const uint32_t* tile_ids;
};
__device__ __forceinline__ void fill_start_args(const RenderArgs& a, StartArgs& o) {
  o.cam = a.cam;
  o.fw1 = a.fw1; o.fh1 = a.fh1; o.rw1 = a.rw1; o.rh1 = a.rh1; o.time_span = a.time_span;
  o.w = a.w; o.h = a.h; o.spp = a.spp; o.max_depth = a.max_depth; o.tiles_x = a.tiles_x;
  o.slot_base = a.slot_base; o.tile_first = a.tile_first; o.tile_stride = a.tile_stride;
  o.spp_magic = a.spp_magic; o.tiles_x_magic = a.tiles_x_magic; o.seed_hash = a.seed_hash;
  o.tile_ids = a.tile_ids;
}

// start_path (below) in two halves, for the start ring's 7-word entry (path_kernel SRING, K.ldsn_ring()): start_make
// is everything up to the time draw -- the scaled lens sample rd, the image coordinates u, v (and the direction d from
// them) and the generator's state before that draw -- and start_take the rest from those: the origin (the lens offset
// again, from the same operands), the direction, the time draw, T, depth and the id.  The same f32 operations on the
// same inputs as start_path's, so every bit of the start is the same.  (A copy, not start_path's own body: with start_path written as the two halves back to back
// every other variant's register allocation moved -- VGPRs, scratch and VALU count, scripts/isa_usage.sh.)
// (The entry keeps u, v instead of d: start_take rebuilds d with start_make's own expression, the same operations in
// the same order on the same bits, and the word this frees holds the start's first hit, below.)
struct StartMade {
  float rdx, rdy;
  float u, v;
  V3 d;
  uint64_t rng;
  uint32_t tile;  // the 64 ids' global tile (wave-uniform: 64 consecutive ids are one sample of one tile)
};
// What a ring entry knows of its path's first segment (the per-tile lists, rtw_tile_beam.h): the closest hit's
// primitive index (>= 0), START_MISS (nothing hit), or START_WALK (not decided: the segment walks the tree)
constexpr int32_t START_MISS = -1, START_WALK = -3;
// The ring entry's winner word: the winner in the low half (RING_WALK for START_WALK: the lists' primitive indices are
// below TILE_LIST_OVER, the same value), the path's lane of origin in the make (id = the ring's first id + it) above.
// A START_MISS path is never stored: the make writes its sample (path_kernel).
constexpr uint32_t RING_WALK = 0xFFFFu;
template <bool FROM_LDS, bool AB>
__device__ __forceinline__ bool start_make(const StartArgs& a, uint64_t pid, StartMade& m) {
  if constexpr (FROM_LDS) asm volatile("" ::: "memory");  // read the LDS copy here: no loop-invariant register copies
  const uint32_t hi = (uint32_t)(pid >> 6), l = (uint32_t)pid & 63u;
  const uint32_t slot = a.spp > 1u ? fastdiv(hi, a.spp_magic) : hi, s = hi - slot * a.spp;
  const uint32_t gslot = a.slot_base + slot;
  const uint32_t tile = a.tile_ids ? a.tile_ids[gslot] : a.tile_first + gslot * a.tile_stride;
  const uint32_t ty = a.tiles_x > 1u ? fastdiv(tile, a.tiles_x_magic) : tile;
  const uint32_t i = (tile - ty * a.tiles_x) * 8u + (l & 7u), row = ty * 8u + (l >> 3);
  // (an off-image id runs through the rest all the same, on a pixel that does not exist, and the caller drops what it
  // made: the wave makes 64 starts together, and results carried out of a divergent branch were spilled to scratch)
  const uint32_t j = a.h - 1u - row;
  const DevCamera& C = a.cam;
  uint64_t rng = xoro_seed(splitmix64(a.seed_hash ^ (((uint64_t)j << 48) | ((uint64_t)i << 32) | s)));
  // lib.rs:84-86 + camera.rs:66-74
  const float u = div_by_recip((float)i + gen_f32(rng), a.fw1, a.rw1);
  const float v = div_by_recip((float)j + gen_f32(rng), a.fh1, a.rh1);
  const V3 rd = scale(rand_in_unit_disk<AB>(rng), C.lens_radius);
  const V3 off = add(scale(ld3(C.u), rd.x), scale(ld3(C.v), rd.y));
  m.rdx = rd.x;
  m.rdy = rd.y;
  m.u = u;
  m.v = v;
  m.tile = tile;
  m.d = sub(sub(add(add(ld3(C.llc), scale(ld3(C.horizontal), u)), scale(ld3(C.vertical), v)), ld3(C.origin)), off);
  m.rng = rng;
  return i < a.w && row < a.h;
}
// (FENCE: the ring's take re-reads the LDS copy of the operands, as start_make does)
template <bool FENCE, bool AB>
__device__ __forceinline__ void start_take(const StartArgs& a, float rdx, float rdy, float u, float v, uint64_t rng,
                                           uint32_t pid, PathState& st) {
  if constexpr (FENCE) asm volatile("" ::: "memory");
  const DevCamera& C = a.cam;
  const V3 off = add(scale(ld3(C.u), rdx), scale(ld3(C.v), rdy));
  st.ray.o = add(ld3(C.origin), off);
  st.ray.d = sub(sub(add(add(ld3(C.llc), scale(ld3(C.horizontal), u)), scale(ld3(C.vertical), v)), ld3(C.origin)), off);
  st.ray.time = gen_range<AB>(rng, C.time0, C.time1, a.time_span);
  st.rng = rng;
  st.T = mk(1.f, 1.f, 1.f);
  st.depth = a.max_depth;
  st.pid = pid;
}

// The ring's make step, after start_make: the first segment's closest hit from the tile's list (RenderArgs::tile_lists),
// with all 64 lanes on.  Every lane finishes its camera ray as start_take will (the time drawn from a copy of the
// generator's state, the origin from the same operands) and folds the always-list and the tile's list with the walks'
// own test_prim and Best: the list holds every BVH primitive a camera ray of the tile can hit (rtw_tile_beam.h), the
// fold is the walk's commutative one (min t, ties to the larger key), so the winner is the walk's.  The list's words
// and the primitives' records come through scalar loads (the tile is wave-uniform).  START_WALK when the render has no
// lists or the tile's list overflowed.
template <bool COUNT, uint32_t FEAT, bool AB>
__device__ __forceinline__ int32_t start_decide(const DevScene& S, const StartArgs& a, const uint32_t* lists,
                                                const StartMade& m, uint32_t* cnt) {
  if (!lists) return START_WALK;  // kernel-uniform
  const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)m.tile);
  // (a caller's tile table may name a tile outside the frame: its ids are all off-image, and it has no record)
  if (tile >= a.tiles_x * ((a.h + 7u) >> 3)) return START_WALK;
  const uint32_t* const rec = lists + (size_t)tile * TILE_LIST_WORDS;
  const uint32_t w0 = uload(rec);
  const uint32_t n = w0 & 0xFFFFu;
  if (n == TILE_LIST_OVER) return START_WALK;  // wave-uniform
  const DevCamera& C = a.cam;
  Ray r;
  const V3 off = add(scale(ld3(C.u), m.rdx), scale(ld3(C.v), m.rdy));
  r.o = add(ld3(C.origin), off);
  r.d = m.d;
  uint64_t g = m.rng;
  r.time = gen_range<AB>(g, C.time0, C.time1, a.time_span);
  const SphRcp rq = sph_rcp(r);
  Best b = Best{INFINITY, 0u, -1, 0.0f, 0.0f};
  for (uint32_t k = 0; k < S.n_always; ++k) test_prim<COUNT, FEAT, false, true>(S, uload(S.always + k), r, b, cnt, g, &rq);
  for (uint32_t k = 1; k <= n; ++k) {  // halfword k of the record
    const uint32_t pi = (uload(rec + (k >> 1)) >> ((k & 1u) * 16u)) & 0xFFFFu;
    test_prim<COUNT, FEAT, false, true>(S, pi, r, b, cnt, g, &rq);
  }
  return b.prim;  // >= 0, or -1 = START_MISS
}

// LST_BLK > 0: also store T = 1, depth and the path id in the lane's LDS state rows (path_kernel LST), here
// where the values are made (carried to the caller, they were spilled)
template <bool FROM_LDS, int LST_BLK = 0, int LST_ROW = 0, bool AB = FROM_LDS>
__device__ __forceinline__ bool start_path(const StartArgs& a, uint64_t pid, PathState& st, uint16_t* lst = nullptr) {
  if constexpr (FROM_LDS) asm volatile("" ::: "memory");  // read the LDS copy here: no loop-invariant register copies
  const uint32_t hi = (uint32_t)(pid >> 6), l = (uint32_t)pid & 63u;
  const uint32_t slot = a.spp > 1u ? fastdiv(hi, a.spp_magic) : hi, s = hi - slot * a.spp;
  const uint32_t gslot = a.slot_base + slot;
  const uint32_t tile = a.tile_ids ? a.tile_ids[gslot] : a.tile_first + gslot * a.tile_stride;
  const uint32_t ty = a.tiles_x > 1u ? fastdiv(tile, a.tiles_x_magic) : tile;
  const uint32_t i = (tile - ty * a.tiles_x) * 8u + (l & 7u), row = ty * 8u + (l >> 3);
  if (i >= a.w || row >= a.h) return false;
  const uint32_t j = a.h - 1u - row;
  const DevCamera& C = a.cam;
  uint64_t rng = xoro_seed(splitmix64(a.seed_hash ^ (((uint64_t)j << 48) | ((uint64_t)i << 32) | s)));
  // lib.rs:84-86 + camera.rs:66-74
  const float u = div_by_recip((float)i + gen_f32(rng), a.fw1, a.rw1);
  const float v = div_by_recip((float)j + gen_f32(rng), a.fh1, a.rh1);
  const V3 rd = scale(rand_in_unit_disk<AB>(rng), C.lens_radius);
  const V3 off = add(scale(ld3(C.u), rd.x), scale(ld3(C.v), rd.y));
  st.ray.o = add(ld3(C.origin), off);
  st.ray.d = sub(sub(add(add(ld3(C.llc), scale(ld3(C.horizontal), u)), scale(ld3(C.vertical), v)), ld3(C.origin)),
                 off);
  st.ray.time = gen_range<AB>(rng, C.time0, C.time1, a.time_span);
  st.rng = rng;
  st.T = mk(1.f, 1.f, 1.f);
  st.depth = a.max_depth;
  st.pid = (uint32_t)pid;
  if constexpr (LST_BLK > 0) {
    const uint32_t v[5] = {0x3F800000u, 0x3F800000u, 0x3F800000u, a.max_depth, (uint32_t)pid};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      lst[(LST_ROW + 2 * k) * LST_BLK] = (uint16_t)v[k];
      lst[(LST_ROW + 2 * k + 1) * LST_BLK] = (uint16_t)(v[k] >> 16);
    }
  }
  return true;
}

// A path kernel's compile-time configuration: path_kernel's template argument, and what the host sizes its launch
// from (Variant).  Everything derived from the fields is defined here, once.
struct KernelCfg {
  int stack;           // LDS stack rows per lane (the branch-free push's extra row not counted)
  bool spill;          // a push bound beyond them goes to HBM (RenderArgs::spill)
  int occ;             // waves per SIMD the register allocator must allow
  uint32_t feat;       // Feature set (rtw_device.hpp), F_LIST for the BVH-less kernels
  int blk = BLOCK;     // workgroup size (256; 448, 512 or 1024 for the LDS-node variants: one copy of the node
                       // table serves the whole workgroup)
  int ncap = 0;        // capacity of the LDS node table in node4s (0 = nodes read from global memory)
  bool half = false;   // the walk reads the half-precision node table (DevNode4h)
  bool s16 = false;    // the global-node walk keeps 16-bit stack entries (trace_run S16)
  // the LDS-node kernel (sorted-push walk over the node table in LDS; no HBM spill path)
  constexpr bool lds_nodes() const { return ncap > 0; }
  // the 1024-lane LDS-node sphere kernel: the LDS its one node table per 16 waves frees holds the waves' start rings
  constexpr bool ldsn_ring() const { return ncap > 0 && blk == 1024 && feat == F_SPHERES; }
  // LST: the S16 mesh walk, and nothing else, keeps the paths' T / depth / id in 10 more 16-bit rows after its stack
  // column's stack + 1 rows (every other kernel has them in PathState)
  constexpr int lst_rows() const { return s16 ? 10 : 0; }
  constexpr int lst_row0() const { return stack + (s16 ? 1 : 0); }
  constexpr bool lst() const { return lst_rows() > 0; }
  constexpr bool shard() const { return ncap > 0; }  // SHARD: several path-id dispensers (path_kernel)
  // SRING: path starts from the wave's ring of 64 (path_kernel; the rect list kernel and the 1024-lane sphere kernel)
  constexpr bool sring() const { return feat == (F_BOXES | F_LIST) || ldsn_ring(); }
  // words per ring entry: the whole start (o, d, time, rng, id), or start_make's half of it where LDS is short
  constexpr int ring_words() const { return ldsn_ring() ? 7 : 10; }
  // the S16 half-node mesh walk keeps the tree's top RTW_MESH_ROOT node4s in LDS (trace_run ROOT)
  constexpr bool root_lds() const { return half && s16 && ncap == 0 && RTW_MESH_ROOT > 0; }
  constexpr bool alignbit_draws() const { return !(feat & F_TRI); }                // AB: the one-alignbit draws
  constexpr bool start_args_in_lds() const { return alignbit_draws() || s16; }     // SLDS (path_kernel)
  constexpr uint32_t node_quads() const { return half ? 7u : 8u; }  // 16-B quads per node (DevNode4h / DevNode4)
  constexpr bool codes16_stack() const { return ncap > 0 || s16; }  // the LDS stack holds 16-bit entries (stk16)
  constexpr int far_lds_nodes() const { return half ? 0 : ncap; }   // trace_far reads f32 nodes: from LDS if there
  // The walk's LDS arrays, in elements (1: unused).  The 32-bit stack columns, + 1: trace_run's branch-free push
  constexpr int stk_words() const { return codes16_stack() ? 1 : (stack + 1) * blk; }
  // the 16-bit stack columns: LDS-node variants STACK rows (window included); S16 (global nodes) STACK + 1 rows and
  // `more` rows after them (path_kernel's LST rows)
  constexpr int stk16_words(int more = 0) const { return ncap > 0 ? stack * blk : (s16 ? (stack + 1 + more) * blk : 1); }
  // the node table (the S16 half-node mesh walk: the tree's top only, trace_run ROOT)
  constexpr uint32_t lds_node_quads() const {
    return ncap > 0 ? ncap * node_quads() : (root_lds() ? RTW_MESH_ROOT * node_quads() : 1u);
  }
};

// The workgroup's copy of the node table into nodes_lds (K.lds_node_quads() quads), before the kernel's first
// __syncthreads(): the whole table (K.ncap > 0) or the tree's top (K.root_lds())
template <KernelCfg K>
__device__ __forceinline__ void fill_nodes_lds(const DevScene& S, float4* nodes_lds) {
  if constexpr (K.ncap > 0) {  // the host launches this variant only when Flat::codes16 and n_nodes <= NCAP
    const float4* g = K.half ? reinterpret_cast<const float4*>(S.hnodes) : reinterpret_cast<const float4*>(S.nodes);
    for (uint32_t k = threadIdx.x; k < S.n_nodes * K.node_quads(); k += K.blk) nodes_lds[k] = g[k];
  }
  if constexpr (K.root_lds()) {
    const uint32_t nq = min(S.n_nodes, (uint32_t)RTW_MESH_ROOT) * K.node_quads();
    if (threadIdx.x < nq) nodes_lds[threadIdx.x] = reinterpret_cast<const float4*>(S.hnodes)[threadIdx.x];
  }
}

template <bool COUNT, KernelCfg K>
__global__ __launch_bounds__(K.blk) __attribute__((amdgpu_waves_per_eu(K.occ, 8))) void path_kernel(RenderArgs a) {
  __shared__ int32_t stk_all[K.stk_words()];
  // LST (the S16 mesh walk): 10 more 16-bit rows after its STACK + 1 hold the path state (below)
  __shared__ uint16_t stk16_all[K.stk16_words(K.lst_rows())];
  __shared__ float4 nodes_lds[K.lds_node_quads()];
  fill_nodes_lds<K>(a.scene, nodes_lds);
  // start_path's operands from LDS in the sphere and list-mode variants (their SGPR spills, and every
  // reload a v_readlane: cornell-800 +6%, jumpy +0.8%) and in the 6 / 7-wave mesh walk (S16): at 80 VGPRs its
  // SGPRs overflowed into VGPR lanes and 28 B per lane of scratch; with the LDS copy 12 B: monument-4k +4.5%,
  // cow-1080p +6.7% (profiles/r05/experiments, m1).  The 5-wave mesh variants keep the kernel arguments (their
  // paths regenerate every ~2 segments: 5-7% slower with the LDS reads in round 3).  The one-alignbit draws (AB)
  // stay with the sphere and list-mode kernels (the triangle kernels' register allocation lost 1-2% with them).
  __shared__ StartArgs start_lds[K.start_args_in_lds() ? 1 : 0 + 1];
  StartArgs sa_reg;
  if constexpr (K.start_args_in_lds()) {
    if (threadIdx.x == 0) fill_start_args(a, start_lds[0]);
  } else {
    fill_start_args(a, sa_reg);
  }
  const StartArgs& SA = K.start_args_in_lds() ? start_lds[0] : sa_reg;
  __syncthreads();
  uint16_t* stk16 = stk16_all + threadIdx.x;
  int32_t* stk = stk_all + threadIdx.x;
  int32_t* spill = a.spill + (size_t)blockIdx.x * K.blk + threadIdx.x;  // unused unless spill_depth > 0
  const uint32_t lane = threadIdx.x & 63u;
  // LST (the S16 mesh walk): a path's throughput, remaining depth and id live in LDS, not VGPRs, which the 6 / 7-wave
  // walk would spill to scratch (a scratch load / store per use in every shading pass).
  // Each 32-bit value is two 16-bit rows of the lane's stack column (rows lst_row0().. + 9: T.x, T.y, T.z,
  // depth, id), addressed from the stack pointer with constant offsets: separate per-lane LDS pointers were
  // loop-invariant VGPRs, which the compiler spilled in turn.
  // (a local copy: with K.lst() in the selects below, the rect list kernels' prologue came out in another order)
  constexpr bool LST = K.lst();
  auto lst_st = [&](int k, uint32_t v) {
    stk16[(K.lst_row0() + 2 * k) * K.blk] = (uint16_t)v;
    stk16[(K.lst_row0() + 2 * k + 1) * K.blk] = (uint16_t)(v >> 16);
  };
  auto lst_ld = [&](int k) -> uint32_t {
    return (uint32_t)stk16[(K.lst_row0() + 2 * k) * K.blk] | ((uint32_t)stk16[(K.lst_row0() + 2 * k + 1) * K.blk] << 16);
  };
  const DevScene& S = a.scene;
  const V3 bg = ld3(a.bg);
  const uint64_t P = a.n_paths;
  // SHARD (the LDS-node sphere kernels): n dispensers (DISP when the host's small-frame rule cut the batch below these
  // kernels' 1024, else 1), 128 B apart: dispenser d hands out the
  // pass's batches d, d + n, d + 2n, ... (interleaved, so the grid still works through the frame in id order, tile
  // after tile), and a wave takes batches from dispenser (its workgroup + k) mod n, k = 0, 1, ... as each runs dry
  // (workgroups are dealt to the XCDs in turn, so each XCD's waves start on their own word).  One word for the whole
  // grid serialises its atomics: the small batches of small passes -- configs[0], an 8-GPU share's short end-of-pass
  // tail -- queued behind it (r06, share8: jumpy's 1/8 share +5%, configs[0] +11%).  The other kernels keep the one
  // word (their code with the dispenser loop ran 1.2-1.8% slower on full frames: cornell, monument).
  unsigned long long* const dispenser = a.queue;
  const uint32_t batch = a.batch, ndisp = batch < 1024u ? DISP : 1u;
  const uint64_t NB = (P + batch - 1u) / batch;  // batches in the pass
  uint32_t cnt[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long nrays = 0;
  // the wave's id pool [next, end) lives in LDS between regenerations: loop-carried 64-bit
  // uniforms otherwise end up as VGPR phis that the 6-wave sphere variant has to spill
  __shared__ uint64_t pool_lds[K.blk / 64][K.shard() ? 5 : 3];
  // S16 mesh walk: the wave index as a scalar, so the pool address is rebuilt from an SGPR (one v_mov) where it is
  // used instead of kept in a VGPR (the 7-wave walk spilled it to scratch and reloaded it at every regeneration;
  // the sphere and list-mode kernels measured 0.5-1.4% slower with it, profiles/r05/experiments s1)
  uint64_t* const pool = pool_lds[K.s16 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : threadIdx.x >> 6];
  if (lane == 0) { pool[0] = 0; pool[1] = 0; }
  if (K.shard() && lane == 0) pool[K.shard() ? 4 : 0] = 0;
  // the wave's next batch [b, e) of path ids (b = e = P: none left); lane 0 takes it, every lane reads it
  auto refill = [&](uint64_t& b, uint64_t& e) {  // (SHARD)
    if (lane == 0) {
      uint64_t bb = P, ee = P;
      uint32_t k = (uint32_t)pool[4];
      for (; k < ndisp; ++k) {
        const uint32_t d = (blockIdx.x + k) & (ndisp - 1u);
        const uint64_t g = atomicAdd(dispenser + d * DISP_STRIDE, 1ull) * ndisp + d;  // the pass's batch g
        if (g < NB) {
          bb = g * batch;
          ee = bb + batch < P ? bb + batch : P;
          break;
        }
      }
      pool[2] = bb;
      pool[K.shard() ? 3 : 0] = ee;
      pool[K.shard() ? 4 : 0] = k;
    }
    b = rfl64(pool[2]);
    e = rfl64(pool[K.shard() ? 3 : 0]);
  };
  // SRING: the wave's ring of 64 path starts, made by all 64 lanes at once from 64 consecutive ids of its pool and
  // taken by the lanes that regenerate (start_path is a function of the id alone, so which lane makes a path's start
  // changes nothing).  start_path at full lane occupancy instead of the few idle lanes of each regeneration.
  // Per lane slot: o, d, time, rng (2 words), pid (10 words, structure of arrays); rng = 0 marks an off-image id.
  // (the rect list kernel: its LDS is free and its VGPRs hold the generation.)
  // The 1024-lane LDS-node sphere kernel (K.ldsn_ring()) has 1.75 KB per wave beside its stack and node table: a 7-word
  // entry, start_make's half of the start -- rd.x, rd.y, u, v, rng before the time draw -- with the first segment's
  // closest hit where the tile's list decides it (start_decide), and the ring's first id once per wave (an entry's id
  // is that + its lane of origin, kept beside the winner); the lanes that take an entry finish it with start_take.
  // The make stores live entries only, packed against the ring's top (head = 64 - their count): an off-image id stores
  // nothing, and a camera ray that the list resolves to a miss is retired by the make itself, which writes its sample
  // and counts its one segment.  A make may so yield fewer entries than the idle lanes want, or none (a sky tile):
  // those lanes stay idle and the wave regenerates again, until its pool and the dispensers are dry.
  // (the other LDS-node and the mesh kernels have no LDS left for a ring at their occupancy)
  // Its head and first id follow the wave's entries (RS words per wave), so one address serves all three.
  constexpr uint32_t RW = K.ring_words(), RS = RW * 64u + (K.ldsn_ring() ? 2u : 0u);
  __shared__ uint32_t ring_lds[K.sring() ? (K.blk / 64) * RS : 1];
  __shared__ uint32_t ring_head_lds[K.sring() && !K.ldsn_ring() ? K.blk / 64 : 1];
  if constexpr (K.ldsn_ring()) {
    // 2 workgroups per CU (8 waves / SIMD at 1024 lanes) share its 163,840 B: 81,920 B each.  16 stack rows x 1024 x
    // 2 B = 32,768 + 144 node4s x 128 B = 18,432 + the ring, 16 waves x 64 entries x 7 words x 4 B = 28,672 + heads and
    // first ids 128 + pools 640 + StartArgs = 80,808 B (a 10-word entry does not fit)
    static_assert(sizeof stk_all + sizeof stk16_all + sizeof nodes_lds + sizeof start_lds + sizeof pool_lds +
                          sizeof ring_lds + sizeof ring_head_lds <= 81920,
                  "the 1024-lane ring kernel's LDS must leave room for 2 workgroups per CU");
  }
  uint32_t* const ring = ring_lds + (K.sring() ? (threadIdx.x >> 6) * RS : 0u);
  uint32_t* const ring_head = K.ldsn_ring() ? ring + RW * 64u : ring_head_lds + (K.sring() ? threadIdx.x >> 6 : 0u);
  uint32_t* const ring_base = ring + (K.ldsn_ring() ? RW * 64u + 1u : 0u);  // (K.ldsn_ring() only)
  if (K.sring() && lane == 0) ring_head[0] = 64u;
  bool exhausted = false;                // wave-uniform
  bool has = false;
  // K.ldsn_ring(): what the lane's ring entry knew of its path's first segment (start_decide), until that segment starts
  int32_t start_win = START_WALK;
  TraceState ts;
  ts.on = false;
  PathState st;
  st.pid = 0;
  st.rng = 0;
  st.depth = 0;
  // COUNT: wave-cycles in regeneration / traversal / shading, then the sub-phases: shading's
  // rejection sampling, traversal's node loop and leaf tests, regeneration's start_path
  uint64_t ph[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // [7..10]: RTW_LANE_DIAG builds only
  const uint64_t t_start = COUNT ? __builtin_amdgcn_s_memtime() : 0;
  uint64_t t_mark = t_start;
  auto phase = [&](int k) {
    if (COUNT) {
      const uint64_t t = __builtin_amdgcn_s_memtime();
      ph[k] += t - t_mark;
      t_mark = t;
    }
  };
  for (;;) {
    phase(2);
    // ---- regeneration: compact new path ids into the idle lanes
    const uint64_t need = __ballot(!has);
    if constexpr (K.sring()) {
      if (need != 0 && !exhausted && ((uint32_t)__popcll(need) >= a.regen_min || need == __ballot(1))) {
        const uint32_t n_need = (uint32_t)__popcll(need);
        const uint32_t rank =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
        const uint64_t t_sp = COUNT ? __builtin_amdgcn_s_memtime() : 0;
        uint32_t head = (uint32_t)__builtin_amdgcn_readfirstlane((int)ring_head[0]);
        const uint32_t have = 64u - head;
        auto take = [&](uint32_t e) {
          if constexpr (K.ldsn_ring()) {  // the 7-word entry: start_take finishes it
            const uint32_t lo = ring[5 * 64 + e], hi = ring[6 * 64 + e];
            const float rdx = __uint_as_float(ring[e]), rdy = __uint_as_float(ring[64 + e]);
            const uint32_t ww = ring[4 * 64 + e];  // winner | lane of origin << 16
            start_take<true, K.alignbit_draws()>(SA, rdx, rdy, __uint_as_float(ring[2 * 64 + e]),
                                                 __uint_as_float(ring[3 * 64 + e]), ((uint64_t)hi << 32) | lo,
                                                 ring_base[0] + (ww >> 16), st);
            start_win = (ww & 0xFFFFu) == RING_WALK ? START_WALK : (int32_t)(ww & 0xFFFFu);
            has = true;  // the ring holds live entries only
          } else {
            const uint32_t lo = ring[7 * 64 + e], hi = ring[8 * 64 + e];
            st.ray.o = mk(__uint_as_float(ring[e]), __uint_as_float(ring[64 + e]), __uint_as_float(ring[2 * 64 + e]));
            st.ray.d = mk(__uint_as_float(ring[3 * 64 + e]), __uint_as_float(ring[4 * 64 + e]),
                          __uint_as_float(ring[5 * 64 + e]));
            st.ray.time = __uint_as_float(ring[6 * 64 + e]);
            st.rng = ((uint64_t)hi << 32) | lo;
            st.pid = ring[9 * 64 + e];
            st.T = mk(1.f, 1.f, 1.f);
            st.depth = SA.max_depth;
            has = (lo | hi) != 0u;
          }
        };
        const bool first = !has && rank < have;
        if (first) take(head + rank);
        if (n_need > have) {  // the ring is spent: 64 more starts from the pool (refilled by one atomic per batch)
          uint64_t pool_next = rfl64(pool[0]), pool_end = rfl64(pool[1]);
          if (pool_next >= pool_end) {
            if constexpr (K.shard()) {
              refill(pool_next, pool_end);
            } else {
              if (lane == 0) pool[2] = atomicAdd(dispenser, (unsigned long long)batch);
              const uint64_t b = rfl64(pool[2]);
              pool_next = b < P ? b : P;
              pool_end = b < P ? (b + batch < P ? b + batch : P) : P;
            }
          }
          // pools and passes hold whole multiples of 64 ids: the host rounds every batch size to one (batch_ids in
          // enqueue_render; the automatic halving stays on powers of two >= 128) and n_paths = slots x 64 x spp
          if (pool_next < pool_end) {
            const uint64_t id = pool_next + lane;
            [[maybe_unused]] uint32_t n_made = 64u;  // K.ldsn_ring(): the entries this make stores (wave-uniform)
            if constexpr (K.ldsn_ring()) {
              StartMade m;
              const bool ok = start_make<K.start_args_in_lds(), K.alignbit_draws()>(SA, id, m);
              const int32_t win = start_decide<COUNT, K.feat, K.alignbit_draws()>(S, SA, a.tile_lists, m, cnt);
              // a camera ray that hits nothing is finished here: its sample is the miss branch's T * bg with T = 1, one
              // segment; the wave's 64 ids are consecutive, so a sky tile's samples are 768 contiguous bytes
              const bool sky = ok && win == START_MISS;
              if (sky) {
                const V3 L = mul(mk(1.f, 1.f, 1.f), bg);
                float* o = a.sbuf + (size_t)(uint32_t)id * 3u;
#if RTW_NT_SAMPLES
                __builtin_nontemporal_store(L.x, o);
                __builtin_nontemporal_store(L.y, o + 1);
                __builtin_nontemporal_store(L.z, o + 2);
#else
                o[0] = L.x;
                o[1] = L.y;
                o[2] = L.z;
#endif
              }
              nrays += (unsigned long long)__popcll(__ballot(sky));
              // the live entries (on the image, not retired) packed against the ring's top: head = 64 - n_live
              const bool live = ok && !sky;
              const uint64_t lv = __ballot(live);
              n_made = (uint32_t)__popcll(lv);
              const uint32_t e = 64u - n_made +
                                 __builtin_amdgcn_mbcnt_hi((uint32_t)(lv >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lv, 0u));
              if (live) {
                ring[e] = __float_as_uint(m.rdx);
                ring[64 + e] = __float_as_uint(m.rdy);
                ring[2 * 64 + e] = __float_as_uint(m.u);
                ring[3 * 64 + e] = __float_as_uint(m.v);
                // (an always-list winner past 16 bits walks instead: the lists' own primitives are below RING_WALK)
                ring[4 * 64 + e] = ((uint32_t)win < RING_WALK ? (uint32_t)win : RING_WALK) | (lane << 16);
                ring[5 * 64 + e] = (uint32_t)m.rng;
                ring[6 * 64 + e] = (uint32_t)(m.rng >> 32);
              }
              if (lane == 0) ring_base[0] = (uint32_t)pool_next;
            } else {
              PathState g;
              const bool ok = start_path<K.start_args_in_lds(), 0, 0, K.alignbit_draws()>(SA, id, g);
              ring[lane] = __float_as_uint(g.ray.o.x);
              ring[64 + lane] = __float_as_uint(g.ray.o.y);
              ring[2 * 64 + lane] = __float_as_uint(g.ray.o.z);
              ring[3 * 64 + lane] = __float_as_uint(g.ray.d.x);
              ring[4 * 64 + lane] = __float_as_uint(g.ray.d.y);
              ring[5 * 64 + lane] = __float_as_uint(g.ray.d.z);
              ring[6 * 64 + lane] = __float_as_uint(g.ray.time);
              ring[7 * 64 + lane] = ok ? (uint32_t)g.rng : 0u;
              ring[8 * 64 + lane] = ok ? (uint32_t)(g.rng >> 32) : 0u;
              ring[9 * 64 + lane] = (uint32_t)id;
            }
            pool_next += 64u;
            // (K.ldsn_ring(): a make may yield fewer than the takers want, or none: they stay idle, and the wave
            // regenerates again under the usual rule)
            if constexpr (K.ldsn_ring()) {
              const uint32_t head0 = 64u - n_made, want = n_need - have;
              if (!has && !first && rank - have < n_made) take(head0 + (rank - have));
              head = head0 + (want < n_made ? want : n_made);
            } else {
              if (!has && !first) take(rank - have);
              head = n_need - have;
            }
          } else {
            exhausted = true;  // no ids left: the ring stays empty
            head = 64u;
          }
          if (lane == 0) { pool[0] = pool_next; pool[1] = pool_end; }
        } else {
          head += n_need;
        }
        if (lane == 0) ring_head[0] = head;
        if (COUNT) ph[6] += __builtin_amdgcn_s_memtime() - t_sp;  // wave-uniform
      }
    } else if (need != 0 && !exhausted && ((uint32_t)__popcll(need) >= a.regen_min || need == __ballot(1))) {
      const uint32_t n_need = (uint32_t)__popcll(need);
      const uint32_t rank =
          __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
      uint64_t pool_next = rfl64(pool[0]), pool_end = rfl64(pool[1]);
      const uint64_t avail = pool_end - pool_next;
      uint64_t nb = P, ne = P;
      if (avail < n_need) {  // refill: one atomic per BATCH paths
        // lane 0 takes BATCH ids and hands them to the wave through LDS (a `b = 0` default
        // for the other lanes would be one more loop-carried VGPR pair)
        if constexpr (K.shard()) {
          uint64_t b, e;
          refill(b, e);
          if (b < e) {
            nb = b;
            ne = e;
          } else {
            exhausted = true;
          }
        } else {
          if (lane == 0) pool[2] = atomicAdd(dispenser, (unsigned long long)batch);
          const uint64_t b = rfl64(pool[2]);
          if (b < P) {
            nb = b;
            ne = b + batch < P ? b + batch : P;
          } else {
            exhausted = true;
          }
        }
      }
      const uint64_t t_sp = COUNT ? __builtin_amdgcn_s_memtime() : 0;
      if (!has) {
        const uint64_t id = rank < avail ? pool_next + rank : nb + (rank - avail);
        if ((rank < avail || id < ne) &&
            start_path<K.start_args_in_lds(), LST ? K.blk : 0, K.lst_row0(), K.alignbit_draws()>(SA, id, st, stk16)) {
          has = true;
        }
      }
      if (COUNT) ph[6] += __builtin_amdgcn_s_memtime() - t_sp;  // wave-uniform
      if (avail >= n_need) {
        pool_next += n_need;
      } else {
        pool_next = nb + (n_need - avail);
        pool_end = ne;
        if (pool_next > pool_end) pool_next = pool_end;
      }
      if (lane == 0) { pool[0] = pool_next; pool[1] = pool_end; }
    }
    // (before the empty-round exits: a round that starts no path, a wave's last one included, is regeneration time
    // too; marked after them it fell to shading, and the path_start share could exceed regeneration's)
    phase(0);
    if (__ballot(has) == 0) {
      if (exhausted) break;
      continue;  // every id handed out this round was an off-image pixel: draw again
    }
    // segments starting now, counted per wave with every lane active (so the count is uniform
    // and stays in SGPRs)
    nrays += (unsigned long long)__popcll(__ballot(has && !ts.on));
    if (!has) continue;
    // ---- one segment: closest hit (resumable) + shading (lib.rs:97-117)
    bool decided = false;  // K.ldsn_ring(): the segment starting now has its hit from the ring (no walk)
    if (!ts.on) {
      if constexpr (K.ldsn_ring()) {
        decided = start_win != START_WALK;
        trace_begin<COUNT, K.feat, K.stack, K.blk, K.codes16_stack(), K.far_lds_nodes(), true>(
            S, st.ray, ts, cnt, st.rng, stk16, stk, a.err, nodes_lds, start_win);
        start_win = START_WALK;
      } else {
        trace_begin<COUNT, K.feat, K.stack, K.blk, K.codes16_stack(), K.far_lds_nodes()>(S, st.ray, ts, cnt, st.rng, stk16,
                                                                                         stk, a.err, nodes_lds);
      }
    }
    if (!(K.feat & F_LIST)) {
      const uint32_t act = (uint32_t)__popcll(__ballot(1));
      // lanes whose segment is decided are done on entry: they stay out of the quota's base, which is a share of the
      // lanes that walk
      const uint32_t ndec = K.ldsn_ring() ? (uint32_t)__popcll(__ballot(decided)) : 0u;
      const uint32_t quota = (((act - ndec) * a.quota16 + 15u) >> 4) + ndec;
      const uint32_t leaf_thr = (act * a.leaf16 + 15u) >> 4;
      trace_run<COUNT, K.stack, K.spill, K.feat, K.blk, K.ncap, K.half, K.s16>(S, st.ray, ts, stk, spill, a.spill_lanes, cnt,
                                                                              quota, leaf_thr, st.rng, a.err, ph + 4, nodes_lds, stk16);
    } else {
      ts.node = -1;  // list mode: trace_begin tested every primitive
      ts.sp = 0;
    }
    phase(1);
    __builtin_amdgcn_s_setprio(0);  // trace_run raised it
    if (ts.node >= 0 || ts.sp > 0) continue;  // traversal suspended: resume next iteration
    ts.on = false;
    if (COUNT) simd_tick(cnt, 12, 13);
    const Best b = ts.b;
#ifdef RTW_DIAG_TRACE_PID  // debugging aid (never in the product build): one path's segments via device printf
    if ((RTW_DIAG_TRACE_PID) < 0 || st.pid == (uint32_t)(RTW_DIAG_TRACE_PID))  // < 0: every path
      printf("rtwtrace pid %u o %a %a %a d %a %a %a t %a prim %d key %u rng %016llx\n", st.pid, st.ray.o.x, st.ray.o.y,
             st.ray.o.z, st.ray.d.x, st.ray.d.y, st.ray.d.z, b.t, b.prim, b.prim >= 0 ? S.prims[b.prim].key : 0u,
             (unsigned long long)st.rng);
#endif
    bool done = false;
    V3 L = mk(0.f, 0.f, 0.f);
    // the throughput; the S16 mesh walk reads it from its LDS rows where it is used, after the hit record and the
    // material, so it is not held across them (the 7-wave walk had spilled T.z to scratch there; s1)
    const V3 T0 = st.T;
    auto path_T = [&]() -> V3 {
      return LST ? mk(__uint_as_float(lst_ld(0)), __uint_as_float(lst_ld(1)), __uint_as_float(lst_ld(2))) : T0;
    };
    if (b.prim < 0) {  // lib.rs:102-105
      L = mul(path_T(), bg);
      done = true;
      if (__builtin_expect(b.prim == -2, 0)) {
        // trace_run tripped its guard (a corrupt tree; the frame is invalid and reported): close the path queue
        // for every wave and empty this wave's id pool, so the grid drains after about one trip per wave
        // instead of one per 64 paths (a trip is 2^20 node-loop iterations)
        if constexpr (K.shard()) {
          for (uint32_t d = 0; d < DISP; ++d) atomicMax(dispenser + d * DISP_STRIDE, (unsigned long long)NB);
        } else {
          atomicMax(dispenser, (unsigned long long)P);
        }
        pool[0] = pool[1];
        if constexpr (K.ldsn_ring()) ring_head[0] = 64u;  // and its ring of starts
      }
    } else {
      // the prim's shading record is loaded as soon as the winner is known, beside its geometry
      // (one load instead of the prim -> material -> texture -> checker-child chain)
      // (LST: the second half, the checker's even colour, is read where it is used: held across the hit
      // record it was spilled to scratch)
      DevShade sh;
      if constexpr (LST) {
        const float4 q = *reinterpret_cast<const float4*>(S.shade + b.prim);
        sh.kind = __float_as_uint(q.x); sh.param = q.y; sh.a[0] = q.z; sh.a[1] = q.w;
        sh.a[2] = S.shade[b.prim].a[2];
      } else {
        sh = S.shade[b.prim];
      }
      // a light of one solid colour (light_source.rs:17-24 with SolidColor) needs no hit record: its
      // emission is the colour and it never scatters (the cow's emitting mesh; mesh kernels only: the
      // extra branch measured 0.7% slower on cornell-box)
      const bool solid_light = (K.feat & F_LIGHT) && (K.feat & F_TRI) && (sh.kind & 0xfffu) == (MT_LIGHT | (SM_SOLID << 8));
      Rec h;
      if (!solid_light) h = hit_record<K.feat>(S, st.ray, b, sh.kind);
      else h = Rec{mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 0.f), 0.0f, 0.0f, true, 0u};
#ifdef RTW_SHADE_DIAG  // COUNT-build diagnostic: shading sub-phases (hit record, unit + texture, scatter) in ph[7..9]
      phase(7);
#endif
      // the materials' one body (rtw_dev_shade.hpp), the rejection draw and unit() between its pieces
      const MatKind kind = mat_kind<K.feat>(sh.kind);
      V3 rs = mk(0.f, 0.f, 0.f);
      phase(2);
      if (kind.lam || kind.met || kind.iso) rs = rand_in_unit_sphere<K.alignbit_draws()>(st.rng);  // vec3.rs:101-108
      phase(3);
      const V3 ud = unit(kind.lam ? rs : st.ray.d);  // Lambertian: unit(rs); else unit(d_in)
      // (LST: the checker's even colour from the table, see above)
      const V3 att = mat_attenuation<K.feat>(S, sh, kind, h, [&] { return ld3(LST ? S.shade[b.prim].b : sh.b); });
#ifdef RTW_SHADE_DIAG
      phase(8);
#endif
      V3 Tn = mk(0.f, 0.f, 0.f);  // the throughput after this segment (scattering materials)
      if (kind.light) {  // emit, no scatter
        L = mul(path_T(), att);
        done = true;
      } else {
        const V3 dir = mat_direction<K.feat>(sh, kind, h, ud, rs, st.rng, done);  // done: absorbed
        const V3 Tp = path_T();
        const V3 T2 = mul(Tp, att);  // x * 1.0f == x: the Dielectric's T is unchanged
        // an absorbed Metal ray returns emitted() = black (material.rs:87, lib.rs:109-110), which the recursion's
        // parents multiply by their attenuations: T * 0, not a constant 0 (NaN / inf throughputs propagate, a
        // negative one gives -0; round 6, a fuzz world whose sphere uv was NaN)
        if (done) L = mul(Tp, mk(0.f, 0.f, 0.f));
        Tn = T2;
        if constexpr (LST) {
          lst_st(0, __float_as_uint(T2.x));
          lst_st(1, __float_as_uint(T2.y));
          lst_st(2, __float_as_uint(T2.z));
        } else {
          st.T = T2;
        }
        st.ray.o = h.p;
        st.ray.d = dir;
      }
#ifdef RTW_SHADE_DIAG
      phase(9);
#endif
      if (!done) {  // lib.rs:98-100: depth 0 returns black, times the attenuations above it (T * 0, as above)
        if constexpr (LST) {
          const uint32_t d = lst_ld(3) - 1u;
          lst_st(3, d);
          done = d == 0u;
        } else {
          done = --st.depth == 0u;
        }
        if (done) L = mul(Tn, mk(0.f, 0.f, 0.f));
      }
    }
    if (done) {
      float* o = a.sbuf + (size_t)(LST ? lst_ld(4) : st.pid) * 3u;  // one path's 12 B share a cache line
#ifdef RTW_DIAG_NO_STORE  // timing diagnostic only: what the sample stores (and the waits behind them) cost
      if (L.x == -1.2345f) o[0] = L.y;  // (keeps L live; never true for a finite non-negative radiance)
#else
#if RTW_NT_SAMPLES
      // streaming stores: the 12.7 GB of samples per frame should not evict the scene tables and the
      // register spill lines from L2 (they are read back once, by reduce_kernel)
      __builtin_nontemporal_store(L.x, o);
      __builtin_nontemporal_store(L.y, o + 1);
      __builtin_nontemporal_store(L.z, o + 2);
#else
      o[0] = L.x;
      o[1] = L.y;
      o[2] = L.z;
#endif
#endif  // RTW_DIAG_NO_STORE
      has = false;
    }
  }
  if (lane == 0 && nrays) atomicAdd(a.counters, nrays);  // nrays counts the whole wave's segments
  if (COUNT) {
    phase(2);
    if (lane == 0) {
      for (int k = 0; k < 3; ++k) atomicAdd(a.counters + 16 + k, (unsigned long long)ph[k]);
      atomicAdd(a.counters + 19, (unsigned long long)(t_mark - t_start));
#if defined(RTW_LANE_DIAG) || defined(RTW_UNI_DIAG) || defined(RTW_SHADE_DIAG)
      for (int k = 7; k < 11; ++k) atomicAdd(a.counters + 13 + k, (unsigned long long)ph[k]);
#else
      for (int k = 3; k < 7; ++k) atomicAdd(a.counters + 17 + k, (unsigned long long)ph[k]);
#endif
    }
    for (int q = 0; q < 15; ++q) {
      unsigned long long c = cnt[q];
      for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
      if (lane == 0 && c) atomicAdd(a.counters + 1 + q, c);
    }
  }
}

}  // namespace dev
}  // namespace rtw
