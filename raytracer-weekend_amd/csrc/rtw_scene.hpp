// rtw_scene.hpp — host-side scene graph behind the rtw_* builder calls.
//
// The graph keeps the reference's Hittable tree shape (raytracer_weekend_lib/src/hittable/,
// bvh.rs) so that rtw_scene_dump() can hand the exact hierarchy to the test oracle; the
// flattener (rtw_flatten.cpp) turns it into the device layout of rtw_device.hpp.  Below it: the scene's device
// copies, and what the host sources that call HIP share (the check macro, the device guard, Frame, TileSet, the frame
// checks of the render and camera-ray calls) -- rtw_render.cpp, rtw_query.cpp, rtw_multi.cpp and rtw_kernel.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/rtw.h"
#include "rtw_device.hpp"

struct rtw_scene;  // opaque in the C-ABI; defined below as rtw::Scene's holder

namespace rtw {

enum NodeKind : uint32_t {
  NK_LIST,       // Vec<Box<dyn Hittable>>              hittable/mod.rs:57-69
  NK_BVH,        // BvhNode::new(objects, t0, t1)       bvh.rs:19-74 (set semantics)
  NK_TRANSLATE,  // Translation                         transformations.rs:16-47
  NK_ROTY,       // YRotation                           transformations.rs:50-148
  NK_SPHERE,     // Sphere                              spherical.rs:79-104
  NK_MSPHERE,    // MovingSphere                        spherical.rs:106-151
  NK_RECT,       // XY/XZ/YZRectangle                   rectangular.rs:16-166
  NK_CUBOID,     // Cuboid (six rects)                  rectangular.rs:170-245
  NK_TRI,        // Triangle                            triangular.rs:33-149
  NK_MEDIUM,     // ConstantMedium(boundary, density)   volumes.rs:17-83 (f[0] density, mat = Isotropic)
};

struct Node {
  NodeKind kind;
  std::vector<uint32_t> ch;  // children (groups / wrappers)
  float f[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t axis = 0, mat = 0, tri = 0;
  float sin_t = 0.f, cos_t = 1.f;  // YRotation, computed as transformations.rs:60-63
};

struct TexH {
  uint32_t type = TT_SOLID, odd = 0, even = 0;
  float c[3] = {0, 0, 0};
  float freq = 0.f;
  uint32_t w = 0, h = 0;
  std::vector<uint8_t> img;
  std::vector<float> grad;     // noise: 256 x 3 gradients (perlin.rs:16-19)
  std::vector<uint32_t> perm;  // noise: 3 x 256 permutations (perlin.rs:21-23)
};

struct MatH {
  uint32_t type = MT_LAMBERT, tex = 0;
  float albedo[3] = {0, 0, 0};
  float param = 0.f;
};

// Flattened host copy of what goes to every device.
struct Flat {
  std::vector<DevNode> nodes;    // SAH BVH2 (build + self-check)
  std::vector<DevNode4> nodes4;  // what the kernel walks
  uint32_t stack_need = 0;       // worst-case traversal stack entries of nodes4
  bool codes16 = false;          // DevNode4::code holds valid 16-bit child codes (LDS-node kernels)
  uint32_t stack_need4 = 0;      // the same for the sorted-push walk of the LDS-node kernels (window of 4)
  std::vector<DevNode4h> nodes4h;  // nodes4 in half precision (when codes16; rtw_device.hpp)
  std::vector<DevPrim> prims;
  std::vector<DevShade> shade;  // per prim: material + common texture values (rtw_device.hpp)
  std::vector<DevShade> mshade;  // the same record per material: shade[k] = mshade[prims[k].mat] (rtw_scatter_rays)
  std::vector<uint32_t> always;
  std::vector<float> pboxes;  // per BVH prim (prims[0 .. n_bvh)): its padded, swept box, 8 floats (lo, 0, hi, 0)
  std::vector<DevTriShade> tshade;
  std::vector<DevInst> insts;
  std::vector<DevMat> mats;
  std::vector<DevTex> texs;
  std::vector<uint8_t> texels;
  std::vector<DevPerlin> perlins;
  uint32_t depth = 0;
  uint32_t features = 0;  // Feature bits actually used
  uint32_t msphere_unit = 1;  // every moving sphere has the shutter [+0, 1] (DevPrim::aux)
  uint32_t uni_inst = 0;      // the only instance, a single Translation (0 = none such)
  uint32_t rect_fast = 0;     // DevScene::rect_fast
  std::vector<DevGroup> lgroups;  // DevScene::lgroups
  uint32_t bvh_tri = 0;       // every BVH leaf is a triangle of wrapper chain tri_inst (DevScene::bvh_tri)
  uint32_t tri_inst = 0;
  float uni_off[3] = {0, 0, 0};
  float time_lo = 0.f, time_hi = 1.f;  // shutter interval the moving-sphere boxes cover
  // the far-origin bound of the BVH's sphere tests (rtw_flatten.cpp far_bound; DevScene::far_*)
  uint32_t far_check = 0;
  DevFar far{};
  float far_d0 = 0.f;
};

struct DevBuf {  // a grow-only device allocation
  void* p = nullptr;
  size_t cap = 0;
};

// A kernel's resident capacity on a device (blocks per CU x CUs), kept for the kernel it was computed for: knobs may
// switch a scene's variant between calls (rtw_kernel.hip resident_blocks)
struct ResidentGrid {
  const void* fn = nullptr;
  int blocks = 0;
};
enum GridSlot {
  GRID_PATH, GRID_PATH_COUNT, GRID_HIT, GRID_SCATTER, GRID_CAMERA, GRID_SAMPLE, GRID_FEATURE, GRID_OCCLUDED, GRID_AO, GRID_SLOTS
};

struct DeviceCopy {
  int device = -1;  // the logical device the caller names (rtw_render_device, rtw_render_multi's device d)
  int phys = -1;    // the HIP device it lives on: = device, except under rtw_diag_alias_devices (all on 0)
  void* block = nullptr;  // one hipMalloc holding every table
  size_t bytes = 0;
  DevScene scene{};
  unsigned long long* counters = nullptr;  // COUNTER_WORDS x u64: [0..31] stats, then the path-id dispensers
  // host-mapped sticky error word (hipHostMalloc): a path kernel whose traversal guard trips writes 1;
  // the host reads it at the next render call, rtw_render_status, rtw_path_kernel_times and with stats
  uint32_t* err_host = nullptr;
  DevBuf sbuf;                             // ordered per-sample radiance (rgb floats per path of a pass)
  DevBuf spill;                            // traversal-stack overflow (trees deeper than the LDS stack)
  hipEvent_t kev[64][2] = {};              // pairs around path-kernel launches (ring, rtw_path_kernel_times)
  uint32_t kev_head = 0, kev_count = 0;
  ResidentGrid grids[GRID_SLOTS];          // the path kernel (plain, counting), the five query kernels, the feature and the AO kernel
  // device buffers kept across render calls (grown, never shrunk; freed by release()): a
  // 30-camera animation through rtw_render does no hipMalloc after the first frame
  DevBuf image, tiles, packed, gathered, gather_ids;
  DevBuf feat_albedo, feat_normal, feat_depth;  // rtw_render_features' device sums (grown once)
  DevBuf ao_sums;                          // rtw_render_ao's device sums: (open, cast) per pixel (grown once)
  DevBuf film_sum, film_sq;                // rtw_render_progressive's device sums: the frame's Σ x and Σ x^2
  // rtw_render_adaptive*: two tile-id lists of the frame's tile count and the count word behind them (grown once),
  // the pinned host word the count is read back into, and the host form's per-tile counts and errors
  DevBuf adapt_ids, adapt_tiles;
  uint32_t* adapt_host = nullptr;
  DevBuf qrays, qhits;                     // rtw_hit_rays' staging: one chunk of rays and of records
  DevBuf mshade;                           // Flat::mshade (uploaded with the scene; scatter_kernel's material table)
  DevBuf qscatter;                         // rtw_scatter_rays' staging: one chunk of rtw_scatter records
  DevBuf qsamples;                         // rtw_sample_rays' staging: one chunk of rtw_sample records
  DevBuf qtmax, qoccluded;                 // rtw_occluded_rays' staging beside qrays: one chunk of bounds and of answers
  DevBuf pboxes;                           // Flat::pboxes (uploaded with the scene; tile_list_kernel's box table)
  DevBuf tile_lists;                       // one 32-B record per 8x8 tile of the last frame (tile_list_kernel)
  // the last render on this copy: 1 = its camera rays were resolved from the tile lists; tiles whose list overflowed
  uint32_t lists_used = 0, lists_overflow = 0;
  uint32_t* lists_count = nullptr;         // device word: the list builder's overflow count
  // what c.tile_lists holds: the (camera, size, cap) its records were built for and the stream that built them (a
  // render with the same ones on the same stream reuses them: enqueue_render)
  struct ListsKey {
    rtw_camera cam;
    uint32_t w = 0, h = 0, cap = 0;
    hipStream_t stream = nullptr;
    bool valid = false;
  } lists_key;
  hipEvent_t ev[2] = {nullptr, nullptr};   // pair timing rtw_render / multi calls (copy_events)
  hipStream_t stream = nullptr;            // rtw_render_multi's stream on this device
  hipEvent_t gev[2] = {nullptr, nullptr};  // pair around rtw_render_multi's gather (device 0)
};

struct Scene {
  std::vector<TexH> tex;
  std::vector<MatH> mat;
  std::vector<Node> nodes;        // nodes[0] = world list
  std::vector<uint32_t> open{0};  // open-group stack
  std::vector<float> tri_v, tri_n, tri_uv;  // per triangle: 9, 9, 6 floats (raw inputs)
  std::vector<uint8_t> tri_nm, tri_uvm;     // per triangle: normal / uv presence masks
  bool committed = false;
  bool flattened = false;  // rtw_scene_commit got past the flattener (flat is valid), with or without a device
  Flat flat;
  std::vector<DeviceCopy> dev;
  // the last rtw_render_multi call: per-device render ms (path kernel + in-order reduction) and device 0's
  // gather ms (rtw_render_multi_times)
  std::vector<float> multi_ms;
  float multi_gather_ms = 0.0f;
  // rtw_diag_alias_devices: > 0 = the scene's devices are this many logical devices on physical device 0
  int alias_n = 0;
  Scene() { nodes.push_back(Node{NK_LIST, {}}); }
};

// thread-local error reporting (rtw_capi.cpp)
int fail(int code, const char* fmt, ...);
// A tuning knob's value (RTW_OCC, RTW_BATCH, RTW_LIST_MAX, ...: DESIGN.md §4), or NULL.  The knobs select
// kernel variants and scheduling parameters for A/B measurements; they are read only when RTW_TUNING=1, so a
// process that inherits a stray variable still runs the default (measured-best) kernels.  A knob set without
// the gate is ignored with one warning on stderr (rtw_capi.cpp).
const char* tuning_env(const char* name);

// ---- small things every HIP-calling source shares (rtw_render.cpp, rtw_query.cpp, rtw_multi.cpp, rtw_kernel.hip)
#define HIPCHK(x, what)                                                                        \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess) return rtw::fail(RTW_ENODEV, "%s: %s", what, hipGetErrorString(e_)); \
  } while (0)
// restores the caller's current device on every return path
struct DeviceGuard {
  int prev = 0;
  DeviceGuard() { hipGetDevice(&prev); }
  ~DeviceGuard() { hipSetDevice(prev); }
};
inline int ensure_event(hipEvent_t& e) {  // created at first use, kept (release() destroys it)
  if (!e) HIPCHK(hipEventCreate(&e), "hipEventCreate");
  return RTW_OK;
}
inline hipStream_t abi_stream(void* s) { return (hipStream_t)s; }  // the C-ABI's `void* stream` (include/rtw.h)
inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// What a render call renders: the arguments every entry point takes, built once at the extern "C" boundary.
struct Frame {
  const rtw_camera* cam;
  const float* bg;
  uint32_t w, h, spp, max_depth;
  uint64_t seed;
  // host only: the frame's sample s is sample sample_base + s of its pixel.  A multiple of spp, itself a power of two,
  // so that sample_base + s == sample_base ^ s: frame_args folds it into the path key (enqueue_render_samples' blocks)
  uint32_t sample_base = 0;
  uint32_t tiles_x() const { return (w + 7u) / 8u; }
  // 8x8 pixel tiles, ragged edges whole (fits 32 bits for every image the render accepts: sides <= 65536)
  uint64_t tiles() const { return (uint64_t)((w + 7u) / 8u) * ((h + 7u) / 8u); }
  uint64_t paths() const { return (uint64_t)w * h * spp; }
};
// Which 8x8 tiles a render covers and where they go: slot k renders tile ids[k] (a device array), or
// tile first + k * stride without one; the output is packed [slot][64][3] when `packed`, and with
// ids unless `full` (RTW_FLAG_FULL_IMAGE: ids, each tile at its place), else the full w x h image.
struct TileSet {
  const uint32_t* ids = nullptr;
  uint32_t first = 0, stride = 1, n = 0;
  bool packed = false;
  bool full = false;
};

// rtw_flatten.cpp
int flatten(Scene& s);
// rtw_capi.cpp
std::string dump_scene(const Scene& s);
// rtw_render.cpp: the scene's device copies and the render calls' shared opening
int upload(Scene& s, int device);
void release(Scene& s);
DeviceCopy* find_copy(Scene& s, int device);  // device < 0: the first copy
int grow(DevBuf& b, size_t bytes);            // current device; contents not kept
// The render calls' argument checks, in this order: a NULL argument (RTW_EINVAL), an uncommitted scene (RTW_ESTATE),
// an image under 2x2 (RTW_EINVAL).  `out` is the call's image, device pointer or sink.  flattened_serves: the state
// asked for is the ray queries' (rtw_scene_commit got past the flattener, with or without a device), so that the
// progressive calls' later checks answer on a machine without a GPU, where the device copy is the last thing missing.
int check_frame(const rtw_scene* s, const Frame& f, bool out, bool flattened_serves = false);
// The frame checks one by one, each RTW_EINVAL, shared by the render calls (check_frame; enqueue_render, after the
// device copy is found) and rtw_camera_rays*: an image under 2x2, a side over 65536, a shutter that leaves the
// committed motion range
int check_image_min(uint32_t w, uint32_t h);
int check_image_max(uint32_t w, uint32_t h);
int check_shutter(const rtw_camera& cam, const Flat& f);
// find_copy, or NULL with RTW_ENODEV set: "not committed to device <device><hint>", or without a hint (the calls
// that name no device) "no device copy"
DeviceCopy* need_copy(Scene& s, int device, const char* hint = "");
int copy_events(DeviceCopy& c);  // c.ev[0], c.ev[1] exist
// wait for `stream`, read the launch counters and the ev0 -> ev1 time into st
int collect_stats(DeviceCopy& c, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, uint64_t paths, rtw_stats* st);
// RTW_EINVAL (and clears it) if a path kernel on c's device tripped its traversal guard since the last check
int check_guard(DeviceCopy& c);
float recip_rn(float b);  // RN(1 / b) for an integer-valued b in [1, 2^24) (rtw_diag_recip)
// rtw_kernel.hip: what needs the device compiler
// field 0-7 (stack, spill, occ, feat, blk, ncap, half, s16) of the path-kernel configuration the current
// environment selects for the committed scene (rtw_scene_info 16-23); host only, no device needed
int64_t selected_kernel_info(const Scene& s, int field);
// rtw_scene_info 24 (field 0), 25 (field 1): the tile lists of the last render on the first device copy
int64_t last_render_lists(Scene& s, int field);
// enqueue one render (path kernel passes + in-order reductions) on `stream` of c.device, which must be current;
// ev0 / ev1 (or NULL) are recorded around it
int enqueue_render(Scene& s, DeviceCopy& c, const Frame& f, const TileSet& tiles, float* d_out, hipStream_t stream,
                   uint32_t flags, hipEvent_t ev0, hipEvent_t ev1);
// The aligned power-of-two blocks of the sample range [first, first + n), first + n <= 2^31, in ascending order: block
// k = [firsts[k], firsts[k] + 2^log2s[k]) with firsts[k] a multiple of its size, each the largest such block that
// starts where the one before ended and fits the range (greedy: at most SAMPLE_BLOCKS_MAX of them).  -> their number
constexpr uint32_t SAMPLE_BLOCKS_MAX = 62;
uint32_t sample_blocks(uint32_t first, uint32_t n, uint32_t* firsts, uint32_t* log2s);
// enqueue samples [sample_first, sample_first + f.spp) of the tiles' pixels, ADDED in sample order onto what d_sum and
// d_sq (or NULL) hold, on `stream` of c.device, which must be current: enqueue_render's checks, counters and tile lists
// once, then one round of passes per block of sample_blocks, each pass's in-order reduction continuing the sums.
// Nothing is enqueued but the counters' reset for f.spp == 0 or f.max_depth == 0.  The caller has checked the range.
int enqueue_render_samples(Scene& s, DeviceCopy& c, const Frame& f, uint32_t sample_first, const TileSet& tiles,
                           float* d_sum, float* d_sq, hipStream_t stream, uint32_t flags, hipEvent_t ev0,
                           hipEvent_t ev1);
// enqueue rtw_tonemap over device arrays (n_pixels x rgb sums -> n_pixels x rgb8) on `stream` of the current device
int enqueue_tonemap(const float* d_sum, uint32_t n_pixels, uint32_t spp, uint8_t* d_rgb8, hipStream_t stream);
// enqueue the noise test of n_in tiles (d_ids_in, or NULL: tiles 0 .. n_in - 1) of the full-layout sums d_sum / d_sq
// holding `samples` samples per pixel, on `stream` of the current device: tile_noise_kernel (d_err and d_tile_samples by
// global tile id, either may be NULL), then the stable compaction of the ids not converged into d_ids_out (room for
// n_in words, the call's scratch too; it may not overlap d_ids_in) with their number in *d_n_out.  The caller has
// checked the arguments (rtw_tile_noise_device).
int enqueue_tile_noise(const float* d_sum, const float* d_sq, uint32_t w, uint32_t h, const uint32_t* d_ids_in,
                       uint32_t n_in, uint32_t samples, float threshold, float* d_err, uint32_t* d_tile_samples,
                       uint32_t* d_ids_out, uint32_t* d_n_out, hipStream_t stream);
// enqueue rtw_tonemap_tiles over device arrays on `stream` of the current device
int enqueue_tonemap_tiles(const float* d_sum, uint32_t w, uint32_t h, const uint32_t* d_tile_samples, uint8_t* d_rgb8,
                          hipStream_t stream);
// enqueue rtw_denoise over device arrays on `stream` of the current device: the prepare kernel, `iterations` a-trous
// passes and the finish.  d_scratch holds DENOISE_SCRATCH_PER_PIXEL bytes per pixel, 16-byte aligned.  The caller has
// checked the arguments (rtw_denoise_device).  d_count (or NULL): a sample count per pixel in place of `samples` and
// the table (rtw_denoise_counts_device).
constexpr uint64_t DENOISE_SCRATCH_PER_PIXEL = 64;
int enqueue_denoise(const float* d_sum, const float* d_sq, const float* d_albedo, const float* d_normal,
                    const float* d_depth, const float* d_count, uint32_t w, uint32_t h, uint32_t samples,
                    const uint32_t* d_tile_samples, uint32_t iterations, float sigma_l, float sigma_n, float sigma_z,
                    float* d_out, void* d_scratch, hipStream_t stream);
// rtw_temporal's arguments as both of its forms take them (rtw_temporal.cpp's host loops, rtw_temporal_kernel.hpp's
// kernel, which gets the struct by value): the current frame, the history (hist_count NULL: none) and the outputs,
// device or host pointers alike.  A triple out of use is NULL in all three places.
struct TemporalArgs {
  const float *sum, *sq, *albedo, *normal, *depth;  // 3, 3, 3, 3 and 2 floats per pixel
  const uint32_t* tile_samples;                      // per 8x8 tile, or NULL: `samples` everywhere
  const float *hist_sum, *hist_sq, *hist_albedo, *hist_normal, *hist_depth, *hist_count;
  float *out_sum, *out_sq, *out_albedo, *out_normal, *out_depth, *out_count;
  uint32_t w, h, tiles_x, samples;
  float max_history, tol_z, cos_n;
  rtw_camera cam, hist_cam;
};
// enqueue rtw_temporal over device arrays on `stream` of the current device: one kernel, no scratch.  The caller has
// checked the arguments (rtw_temporal_device).
int enqueue_temporal(const TemporalArgs& a, hipStream_t stream);
// enqueue one closest-hit query of n rays (rtw_ray[n] -> rtw_hit[n], device arrays) on `stream` of c.device, which
// must be current; ev0 / ev1 (or NULL) are recorded around the kernel
int enqueue_hit_rays(Scene& s, DeviceCopy& c, uint64_t n, const void* d_rays, void* d_hits, hipStream_t stream,
                     hipEvent_t ev0, hipEvent_t ev1);
// enqueue one occlusion query of n rays (rtw_ray[n], float[n] or NULL -> uint8_t[n], device arrays), likewise
int enqueue_occluded_rays(Scene& s, DeviceCopy& c, uint64_t n, const void* d_rays, const float* d_t_max,
                          uint8_t* d_occluded, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1);
// enqueue Material::scatter + emitted for n (ray, hit record) pairs (device arrays; d_out_rays may be d_rays) on `stream`
// of c.device, which must be current; ev0 / ev1 (or NULL) are recorded around the kernel
int enqueue_scatter_rays(Scene& s, DeviceCopy& c, uint64_t n, const void* d_rays, const void* d_hits, const float* bg,
                         void* d_out_rays, void* d_out_scatter, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1);
// enqueue the camera rays of paths [first, first + n) of frame f (its max_depth and bg unused) into d_rays, likewise;
// the caller has checked the frame and the shutter (rtw_query.cpp camera_rays_check)
int enqueue_camera_rays(DeviceCopy& c, const Frame& f, uint64_t first, uint64_t n, void* d_rays, hipStream_t stream,
                        hipEvent_t ev0, hipEvent_t ev1);
// enqueue sample_ray for n rays (rtw_ray[n] -> rtw_sample[n], device arrays) on `stream` of c.device, which must be
// current: the dispenser and the counters zeroed, then one persistent launch per 2^31 rays; ev0 / ev1 (or NULL) are
// recorded around them.  Afterwards c.counters[0] holds the segments traced.
int enqueue_sample_rays(Scene& s, DeviceCopy& c, uint64_t n, const void* d_rays, const float* bg, uint32_t max_depth,
                        void* d_samples, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1);
// enqueue samples [sample_first, sample_first + n_samples) of the tiles' pixels as first-hit features, ADDED in sample
// order onto what d_albedo, d_normal (3 floats per pixel) and d_depth (2 per pixel) hold (each may be NULL), on `stream`
// of c.device, which must be current: enqueue_render_samples' checks and counters' reset, then one launch of the
// scene's feature kernel.  Afterwards c.counters[0] holds the samples traced.  The caller has checked the range.
int enqueue_features(Scene& s, DeviceCopy& c, const Frame& f, uint32_t sample_first, const TileSet& tiles,
                     float* d_albedo, float* d_normal, float* d_depth, hipStream_t stream, hipEvent_t ev0,
                     hipEvent_t ev1);
// enqueue samples [sample_first, sample_first + f.spp) of the tiles' pixels as ambient occlusion, ADDED in sample order
// onto what d_ao (2 floats per pixel: open, cast) holds, on `stream` of c.device, which must be current: enqueue_features'
// checks and counters' reset, then one launch of the scene's AO kernel (f.bg and f.max_depth unused).  Afterwards
// c.counters[0] holds the camera samples traced and c.counters[1] the AO rays cast.  The caller has checked the range,
// ao_rays (1 .. 256) and radius (> 0).
int enqueue_ao(Scene& s, DeviceCopy& c, const Frame& f, uint32_t sample_first, const TileSet& tiles, uint32_t ao_rays,
               float radius, float* d_ao, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1);
int enqueue_unpack(uint32_t w, uint32_t h, const uint32_t* d_tiles, uint32_t n_tiles, const float* d_packed,
                   float* d_image, hipStream_t stream);

}  // namespace rtw

struct rtw_scene {
  rtw::Scene s;
};
