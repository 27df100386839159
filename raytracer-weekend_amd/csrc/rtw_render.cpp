// rtw_render.cpp — the host render runtime behind the C-ABI's device half: the scene's device copies (upload, release,
// the grow-only buffers), the render calls' shared opening (check_frame, need_copy) and the frame checks it shares with
// the camera-ray calls, statistics, the traversal guard's error word, and the render / status / diagnostic entry points
// of one device.  Plain HIP runtime API: the kernels, which variant a scene runs and how a render is enqueued are
// rtw_kernel.hip's (enqueue_render, enqueue_render_samples, enqueue_tonemap, enqueue_unpack); the six ray-query calls
// are rtw_query.cpp's, the render over several devices rtw_multi.cpp's.  The progressive calls
// (rtw_render_samples_device, rtw_sample_blocks, rtw_render_progressive, rtw_tonemap_device) are here too.  So are the
// adaptive ones (rtw_tile_noise_device, rtw_render_adaptive_device, rtw_render_adaptive, rtw_tonemap_tiles_device): the
// loop of rounds around enqueue_render_samples and enqueue_tile_noise is render_adaptive below.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "../../include/rtw.h"
#include "rtw_scene.hpp"

namespace rtw {

template <class T>
static size_t put(std::vector<uint8_t>& blob, const std::vector<T>& v) {
  size_t off = (blob.size() + 255) & ~(size_t)255;
  blob.resize(off + sizeof(T) * v.size());
  if (!v.empty()) memcpy(blob.data() + off, v.data(), sizeof(T) * v.size());
  return off;
}

int upload(Scene& s, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(RTW_ENODEV, "no HIP device visible (the render core has no CPU fallback)");
  const int nlog = s.alias_n > 0 ? s.alias_n : ndev;  // logical devices (rtw_diag_alias_devices: all on 0)
  if (device >= nlog) return fail(RTW_EINVAL, "device %d >= device count %d", device, nlog);
  const Flat& f = s.flat;
  std::vector<uint8_t> blob;
  // the far-origin record sits DEVFAR_BACK bytes before the prim table (trace_begin derives it from S.prims)
  DevFar far = f.far;
  const size_t o_nodes = put(blob, f.nodes4), o_far = put(blob, std::vector<DevFar>{far});
  size_t o_prims = put(blob, f.prims), o_always = put(blob, f.always);
  if (o_prims - o_far != DEVFAR_BACK) return fail(RTW_EINVAL, "internal: far record not %u B before the prims", DEVFAR_BACK);
  reinterpret_cast<DevFar*>(blob.data() + o_far)->nodes_back = (uint32_t)(o_prims - o_nodes);
  size_t o_tsh = put(blob, f.tshade), o_inst = put(blob, f.insts), o_mat = put(blob, f.mats);
  size_t o_tex = put(blob, f.texs), o_texel = put(blob, f.texels), o_perlin = put(blob, f.perlins);
  size_t o_shade = put(blob, f.shade), o_hnodes = put(blob, f.nodes4h), o_groups = put(blob, f.lgroups);
  blob.resize((blob.size() + 255) & ~(size_t)255);
  int d0 = device >= 0 ? device : 0, d1 = device >= 0 ? device + 1 : nlog;
  DeviceGuard g;
  // one device's copy, built in place in s.dev: release() frees whatever a failed step leaves behind
  auto fill = [&](DeviceCopy& c, int d) -> int {
    const int phys = s.alias_n > 0 ? 0 : d;
    c.device = d;
    c.phys = phys;
    HIPCHK(hipSetDevice(phys), "hipSetDevice");
    c.bytes = blob.size();
    HIPCHK(hipMalloc(&c.block, c.bytes), "hipMalloc(scene)");
    HIPCHK(hipMemcpy(c.block, blob.data(), c.bytes, hipMemcpyHostToDevice), "hipMemcpy(scene)");
    HIPCHK(hipMalloc((void**)&c.counters, COUNTER_WORDS * sizeof(unsigned long long)), "hipMalloc(counters)");
    // the sticky traversal-error word lives in host memory the kernel writes through (coherent,
    // mapped): the host reads it without a device round trip, also for renders it did not wait for
    HIPCHK(hipHostMalloc((void**)&c.err_host, 64, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc(error word)");
    *(volatile uint32_t*)c.err_host = 0u;
    // the per-material shading records (rtw_scatter_rays): a buffer of their own, so the scene block's layout stays
    if (!f.mshade.empty()) {
      if (int e = grow(c.mshade, f.mshade.size() * sizeof(DevShade))) return e;
      HIPCHK(hipMemcpy(c.mshade.p, f.mshade.data(), f.mshade.size() * sizeof(DevShade), hipMemcpyHostToDevice),
             "hipMemcpy(material shading records)");
    }
    // the BVH primitives' padded boxes (the per-tile lists' builder): a buffer of their own, likewise
    if (!f.pboxes.empty()) {
      if (int e = grow(c.pboxes, f.pboxes.size() * sizeof(float))) return e;
      HIPCHK(hipMemcpy(c.pboxes.p, f.pboxes.data(), f.pboxes.size() * sizeof(float), hipMemcpyHostToDevice),
             "hipMemcpy(primitive boxes)");
    }
    HIPCHK(hipMalloc((void**)&c.lists_count, 64), "hipMalloc(tile-list counter)");
    uint8_t* base = (uint8_t*)c.block;
    c.scene.nodes = (const DevNode4*)(base + o_nodes);
    c.scene.hnodes = f.nodes4h.empty() ? nullptr : (const DevNode4h*)(base + o_hnodes);
    c.scene.prims = (const DevPrim*)(base + o_prims);
    c.scene.always = (const uint32_t*)(base + o_always);
    c.scene.tshade = (const DevTriShade*)(base + o_tsh);
    c.scene.insts = (const DevInst*)(base + o_inst);
    c.scene.mats = (const DevMat*)(base + o_mat);
    c.scene.texs = (const DevTex*)(base + o_tex);
    c.scene.texels = (const uint8_t*)(base + o_texel);
    c.scene.perlins = (const DevPerlin*)(base + o_perlin);
    c.scene.shade = (const DevShade*)(base + o_shade);
    c.scene.lgroups = (const DevGroup*)(base + o_groups);
    c.scene.n_lgroups = (uint32_t)f.lgroups.size();
    c.scene.n_nodes = (uint32_t)f.nodes4.size();
    c.scene.n_prims = (uint32_t)f.prims.size();
    c.scene.n_always = (uint32_t)f.always.size();
    c.scene.n_insts = (uint32_t)f.insts.size();
    c.scene.msphere_unit = f.msphere_unit;
    c.scene.uni_inst = f.uni_inst;
    c.scene.bvh_tri = f.bvh_tri;  // knob RTW_TRI_LEAF (rtw_flatten.cpp)
    c.scene.tri_inst = f.tri_inst;
    c.scene.rect_fast = f.rect_fast;
    memcpy(c.scene.uni_off, f.uni_off, sizeof f.uni_off);
    c.scene.far_check = f.far_check;
    return RTW_OK;
  };
  for (int d = d0; d < d1; ++d) {
    s.dev.emplace_back();
    if (int e = fill(s.dev.back(), d)) {
      release(s);
      return e;
    }
  }
  return RTW_OK;
}

static void free_buf(DevBuf& b) {
  if (b.p) hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

void release(Scene& s) {
  for (DeviceCopy& c : s.dev) {
    if (hipSetDevice(c.phys) != hipSuccess) continue;
    if (c.block) hipFree(c.block);
    if (c.counters) hipFree(c.counters);
    if (c.err_host) hipHostFree(c.err_host);
    if (c.lists_count) hipFree(c.lists_count);
    for (DevBuf* b : {&c.sbuf, &c.spill, &c.image, &c.tiles, &c.packed, &c.gathered, &c.gather_ids, &c.qrays, &c.qhits,
                       &c.mshade, &c.qscatter, &c.qsamples, &c.qtmax, &c.qoccluded, &c.pboxes, &c.tile_lists, &c.film_sum, &c.film_sq, &c.feat_albedo, &c.feat_normal, &c.feat_depth, &c.ao_sums,
                       &c.adapt_ids, &c.adapt_tiles})
      free_buf(*b);
    if (c.adapt_host) hipHostFree(c.adapt_host);
    for (hipEvent_t e : {c.ev[0], c.ev[1], c.gev[0], c.gev[1]})
      if (e) hipEventDestroy(e);
    if (c.stream) hipStreamDestroy(c.stream);
    for (auto& pair : c.kev)
      for (hipEvent_t e : pair)
        if (e) hipEventDestroy(e);
  }
  s.dev.clear();
}

DeviceCopy* find_copy(Scene& s, int device) {
  for (DeviceCopy& c : s.dev)
    if (c.device == device || device < 0) return &c;
  return nullptr;
}

int grow(DevBuf& b, size_t bytes) {
  if (bytes <= b.cap) return RTW_OK;
  free_buf(b);
  HIPCHK(hipMalloc(&b.p, bytes), "hipMalloc(render buffer)");
  b.cap = bytes;
  return RTW_OK;
}

int check_frame(const rtw_scene* s, const Frame& f, bool out, bool flattened_serves) {
  if (!s || !f.cam || !f.bg || !out) return fail(RTW_EINVAL, "NULL argument");
  if (!(flattened_serves ? s->s.flattened : s->s.committed)) return fail(RTW_ESTATE, "scene not committed");
  return check_image_min(f.w, f.h);
}

int check_image_min(uint32_t w, uint32_t h) {
  if (w < 2 || h < 2) return fail(RTW_EINVAL, "image must be at least 2x2 (lib.rs:84-85 divides by w-1, h-1)");
  return RTW_OK;
}

int check_image_max(uint32_t w, uint32_t h) {
  if (w > 65536u || h > 65536u)
    return fail(RTW_EINVAL, "image %ux%u: at most 65536 x 65536 (16-bit pixel coordinates in the path key)", w, h);
  return RTW_OK;
}

int check_shutter(const rtw_camera& cam, const Flat& f) {
  if (cam.time0 < f.time_lo || cam.time1 > f.time_hi)
    return fail(RTW_EINVAL, "camera shutter [%g, %g) outside the committed motion range [%g, %g]", cam.time0, cam.time1,
                f.time_lo, f.time_hi);
  return RTW_OK;
}

// the sample calls' range: the sample index is the path key's low word, and a block's size a uint32_t
static int check_sample_range(uint32_t first, uint32_t n) {
  if ((uint64_t)first + n > (1ull << 31))
    return fail(RTW_EINVAL, "samples [%u, %u + %u) go beyond 2^31", first, first, n);
  return RTW_OK;
}

// the feature calls' checks before the sample range: check_frame's (`out`: one of the three buffers is there), with
// the flags between its NULL test and the scene's state
static int check_features(const rtw_scene* s, const Frame& f, bool out, uint32_t flags) {
  if (!s || !f.cam || !f.bg || !out) return fail(RTW_EINVAL, "NULL argument");
  if (flags & ~(uint32_t)RTW_FLAG_FULL_IMAGE) return fail(RTW_EINVAL, "flags %#x: RTW_FLAG_FULL_IMAGE only", flags);
  return check_frame(s, f, out, true);
}

// the AO calls take check_features' opening with their buffer as `out`; they have no background (frame_args copies one)
static const float AO_NO_BG[3] = {0.0f, 0.0f, 0.0f};
// ... then, after the sample range: the AO rays per hit (the sums add (float)K exactly) and the radius (+inf is valid)
static int check_ao(uint32_t ao_rays, float radius) {
  if (ao_rays < 1u || ao_rays > 256u) return fail(RTW_EINVAL, "ao_rays %u: 1 .. 256", ao_rays);
  if (!(radius > 0.0f)) return fail(RTW_EINVAL, "radius %g: must be > 0 (+inf: sky visibility)", (double)radius);
  return RTW_OK;
}
// ao_kernel's two counter words as collect_stats read them (rays <- [0], node_visits <- [1]) -> the AO calls' stats
static void ao_stats(rtw_stats& st) {
  st.paths = st.rays;             // the camera samples traced
  st.rays += st.node_visits;      // ... and the AO rays cast: every world.hit query
  st.node_visits = 0;
}

// the adaptive calls' threshold: err <= threshold must be able to hold and to fail
static int check_threshold(float threshold) {
  if (!(threshold >= 0.0f) || isinf(threshold))
    return fail(RTW_EINVAL, "threshold %g: must be finite and >= 0", (double)threshold);
  return RTW_OK;
}

DeviceCopy* need_copy(Scene& s, int device, const char* hint) {
  DeviceCopy* c = find_copy(s, device);
  if (c) return c;
  if (hint) fail(RTW_ENODEV, "scene was not committed to device %d%s", device, hint);
  else fail(RTW_ENODEV, "scene has no device copy");
  return nullptr;
}

int copy_events(DeviceCopy& c) {
  for (hipEvent_t& e : c.ev)
    if (int rc = ensure_event(e)) return rc;
  return RTW_OK;
}

// RN(1 / b) for an integer-valued b in [1, 2^24): the float nearest 1 / b, chosen among the neighbours of
// the double quotient by the exact residual |1 - y b| (y b is exact in double: 24 x 24 bits)
float recip_rn(float b) {
  float y = (float)(1.0 / (double)b), best = y;
  double e = fabs(1.0 - (double)y * (double)b);
  for (float c : {nextafterf(y, 0.0f), nextafterf(y, 2.0f)}) {
    const double ec = fabs(1.0 - (double)c * (double)b);
    if (ec < e) { e = ec; best = c; }
  }
  return best;
}

int check_guard(DeviceCopy& c) {
  volatile uint32_t* e = c.err_host;
  if (e && *e) {
    *e = 0u;
    return fail(RTW_EINVAL, "a path kernel on device %d tripped its BVH traversal guard (corrupt tree?): the frame "
                "it rendered is invalid", c.device);
  }
  return RTW_OK;
}

int collect_stats(DeviceCopy& c, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, uint64_t paths, rtw_stats* st) {
  HIPCHK(hipStreamSynchronize(stream), "render_kernel");
  unsigned long long cnt[32];
  HIPCHK(hipMemcpy(cnt, c.counters, sizeof cnt, hipMemcpyDeviceToHost), "hipMemcpy(counters)");
  float ms = 0.f;
  if (ev0 && ev1) HIPCHK(hipEventElapsedTime(&ms, ev0, ev1), "hipEventElapsedTime");
  if (int e = check_guard(c)) return e;
  st->rays = cnt[0];
  st->paths = paths;
  st->kernel_ms = ms;
  st->node_visits = cnt[1];
  st->prim_tests = cnt[2];
  for (int k = 0; k < 6; ++k) st->prim_tests_by_type[k] = cnt[3 + k];
  for (int k = 0; k < 6; ++k) st->simd[k] = cnt[9 + k];
  for (int k = 0; k < 4; ++k) st->phase_cycles[k] = cnt[16 + k];
  st->boxes_tested = cnt[15];
  for (int k = 0; k < 4; ++k) st->sub_cycles[k] = cnt[20 + k];
  return RTW_OK;
}

// rtw_render_device and rtw_render_device_strided behind their tile sets
static int render_device(rtw_scene* s, int device, const Frame& f, const TileSet& ts, float* d_out, hipStream_t stream,
                         uint32_t flags, rtw_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  if (int e = check_frame(s, f, d_out)) return e;
  DeviceCopy* c = need_copy(s->s, device);
  if (!c) return RTW_ENODEV;
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  if (stats)
    if (int e = copy_events(*c)) return e;
  const hipEvent_t e0 = stats ? c->ev[0] : nullptr, e1 = stats ? c->ev[1] : nullptr;
  int rc = enqueue_render(s->s, *c, f, ts, d_out, stream, flags, e0, e1);
  if (rc == RTW_OK && stats) {
    rtw_stats st{};
    rc = collect_stats(*c, stream, e0, e1, (uint64_t)ts.n * 64u * f.spp, &st);
    st.total_ms = ms_since(t0);
    *stats = st;
  }
  return rc;
}

// rtw_render_adaptive_device and rtw_render_adaptive behind their checks: c's device is current, the frame's spp is
// max_spp.  Rounds end at n_0 = min_spp, n_{k+1} = min(2 n_k, max_spp); each adds samples [n_{k-1}, n_k) to the tiles
// still active (full layout) and tests them; the list of those not converged is the next round's tile set.
static int render_adaptive(Scene& sc, DeviceCopy& c, const Frame& f, uint32_t min_spp, float threshold, float* d_sum,
                           float* d_sq, uint32_t* d_tile_samples, float* d_tile_err, hipStream_t stream,
                           uint32_t flags, rtw_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  if (int e = check_image_max(f.w, f.h)) return e;
  const uint32_t nt = (uint32_t)f.tiles();
  if (int e = copy_events(c)) return e;
  if (int e = grow(c.adapt_ids, ((size_t)2 * nt + 1) * sizeof(uint32_t))) return e;
  if (!c.adapt_host)
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c.adapt_host), sizeof(uint32_t), hipHostMallocDefault),
           "hipHostMalloc(count)");
  uint32_t* list[2] = {static_cast<uint32_t*>(c.adapt_ids.p), static_cast<uint32_t*>(c.adapt_ids.p) + nt};
  uint32_t* d_count = list[1] + nt;
  const size_t bytes = (size_t)f.w * f.h * 3 * sizeof(float);
  HIPCHK(hipMemsetAsync(d_sum, 0, bytes, stream), "hipMemsetAsync(sums)");
  HIPCHK(hipMemsetAsync(d_sq, 0, bytes, stream), "hipMemsetAsync(sums of squares)");
  rtw_stats tot{};
  const uint32_t* active = nullptr;  // the first round: every tile, no table
  uint32_t n_active = nt, done = 0;
  for (uint32_t round = 0; n_active && done < f.spp; ++round) {
    const uint32_t end = done ? (uint32_t)std::min<uint64_t>(2ull * done, f.spp) : min_spp;
    Frame chunk = f;
    chunk.spp = end - done;
    TileSet ts{active, 0, 1, n_active};
    ts.full = true;
    if (int e = enqueue_render_samples(sc, c, chunk, done, ts, d_sum, d_sq, stream, flags, c.ev[0], nullptr)) return e;
    uint32_t* next = list[round & 1u];
    if (int e = enqueue_tile_noise(d_sum, d_sq, f.w, f.h, active, n_active, end, threshold, d_tile_err, d_tile_samples,
                                   next, d_count, stream))
      return e;
    HIPCHK(hipEventRecord(c.ev[1], stream), "hipEventRecord");
    HIPCHK(hipMemcpyAsync(c.adapt_host, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
           "hipMemcpyAsync(count)");
    rtw_stats st{};
    if (stats) {
      if (int e = collect_stats(c, stream, c.ev[0], c.ev[1], 0, &st)) return e;
    } else {
      HIPCHK(hipStreamSynchronize(stream), "render_kernel");
      if (int e = check_guard(c)) return e;
    }
    tot.rays += st.rays;
    tot.kernel_ms += st.kernel_ms;
    tot.node_visits += st.node_visits;
    tot.prim_tests += st.prim_tests;
    tot.paths += (uint64_t)n_active * 64u * (end - done);
    done = end;
    active = next;
    n_active = *static_cast<volatile uint32_t*>(c.adapt_host);
  }
  tot.total_ms = ms_since(t0);
  if (stats) *stats = tot;
  return RTW_OK;
}

// the adaptive render calls' checks after check_frame, before the device copy
static int check_adaptive(uint32_t min_spp, uint32_t max_spp, float threshold) {
  if (min_spp < 2u || min_spp > max_spp || max_spp > (1u << 31))
    return fail(RTW_EINVAL, "min_spp %u, max_spp %u: 2 <= min_spp <= max_spp <= 2^31", min_spp, max_spp);
  return check_threshold(threshold);
}

}  // namespace rtw

using namespace rtw;

extern "C" {

int rtw_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int rtw_render(rtw_scene* s, const rtw_camera* cam, const float bg[3], uint32_t w, uint32_t h,
               uint32_t spp, uint32_t max_depth, uint64_t seed, float* out, rtw_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  const Frame f{cam, bg, w, h, spp, max_depth, seed};
  if (int e = check_frame(s, f, out)) return e;
  DeviceCopy* c = need_copy(s->s, -1, nullptr);
  if (!c) return RTW_ENODEV;
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  const size_t bytes = (size_t)w * h * 3 * sizeof(float);
  if (int e = copy_events(*c)) return e;
  if (int e = grow(c->image, bytes)) return e;  // kept for the next frame (no per-call hipMalloc)
  float* d_out = static_cast<float*>(c->image.p);
  rtw_stats st{};
  const TileSet all{nullptr, 0, 1, (uint32_t)f.tiles()};
  int rc = enqueue_render(s->s, *c, f, all, d_out, nullptr, 0, c->ev[0], c->ev[1]);
  if (rc == RTW_OK) rc = collect_stats(*c, nullptr, c->ev[0], c->ev[1], f.paths(), &st);
  if (rc == RTW_OK && hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(RTW_ENODEV, "hipMemcpy(image)");
  st.total_ms = ms_since(t0);
  if (stats) *stats = st;
  return rc;
}

int rtw_render_device(rtw_scene* s, int device, const rtw_camera* cam, const float bg[3], uint32_t w,
                      uint32_t h, uint32_t spp, uint32_t max_depth, uint64_t seed, const uint32_t* d_tiles,
                      uint32_t n_tiles, float* d_out, void* stream, uint32_t flags, rtw_stats* stats) {
  const Frame f{cam, bg, w, h, spp, max_depth, seed};
  const TileSet ts{d_tiles, 0, 1, d_tiles ? n_tiles : (uint32_t)f.tiles()};
  return render_device(s, device, f, ts, d_out, abi_stream(stream), flags, stats);
}

int rtw_render_device_strided(rtw_scene* s, int device, const rtw_camera* cam, const float bg[3], uint32_t w,
                              uint32_t h, uint32_t spp, uint32_t max_depth, uint64_t seed, uint32_t first_tile,
                              uint32_t tile_stride, uint32_t n_tiles, float* d_out, void* stream, uint32_t flags,
                              rtw_stats* stats) {
  const Frame f{cam, bg, w, h, spp, max_depth, seed};
  const uint64_t nt = f.tiles();
  if (tile_stride == 0 || (n_tiles && first_tile + (uint64_t)(n_tiles - 1) * tile_stride >= nt))
    return fail(RTW_EINVAL, "tiles %u + k * %u (k < %u) leave the frame's %llu tiles", first_tile, tile_stride, n_tiles,
                (unsigned long long)nt);
  const TileSet ts{nullptr, first_tile, tile_stride, n_tiles, true};
  return render_device(s, device, f, ts, d_out, abi_stream(stream), flags, stats);
}

int rtw_render_samples_device(rtw_scene* s, int device, const rtw_camera* cam, const float bg[3], uint32_t w,
                              uint32_t h, uint32_t sample_first, uint32_t n_samples, uint32_t max_depth,
                              uint64_t seed, const uint32_t* d_tiles, uint32_t n_tiles, float* d_sum, float* d_sq,
                              void* stream, uint32_t flags, rtw_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  const Frame f{cam, bg, w, h, n_samples, max_depth, seed};
  if (int e = check_frame(s, f, d_sum, true)) return e;
  if (int e = check_sample_range(sample_first, n_samples)) return e;
  DeviceCopy* c = need_copy(s->s, device);
  if (!c) return RTW_ENODEV;
  TileSet ts{d_tiles, 0, 1, d_tiles ? n_tiles : (uint32_t)f.tiles()};
  ts.full = (flags & RTW_FLAG_FULL_IMAGE) != 0;
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  if (stats)
    if (int e = copy_events(*c)) return e;
  const hipEvent_t e0 = stats ? c->ev[0] : nullptr, e1 = stats ? c->ev[1] : nullptr;
  const hipStream_t st = abi_stream(stream);
  int rc = enqueue_render_samples(s->s, *c, f, sample_first, ts, d_sum, d_sq, st, flags, e0, e1);
  if (rc == RTW_OK && stats) {
    rtw_stats out{};
    rc = collect_stats(*c, st, e0, e1, (uint64_t)ts.n * 64u * n_samples, &out);
    out.total_ms = ms_since(t0);
    *stats = out;
  }
  return rc;
}

int rtw_render_features_device(rtw_scene* s, int device, const rtw_camera* cam, const float bg[3], uint32_t w,
                               uint32_t h, uint32_t sample_first, uint32_t n_samples, uint64_t seed,
                               const uint32_t* d_tiles, uint32_t n_tiles, float* d_albedo, float* d_normal,
                               float* d_depth, void* stream, uint32_t flags, rtw_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  const Frame f{cam, bg, w, h, n_samples, 1, seed};
  if (int e = check_features(s, f, d_albedo || d_normal || d_depth, flags)) return e;
  if (int e = check_sample_range(sample_first, n_samples)) return e;
  DeviceCopy* c = need_copy(s->s, device);
  if (!c) return RTW_ENODEV;
  TileSet ts{d_tiles, 0, 1, d_tiles ? n_tiles : (uint32_t)f.tiles()};
  ts.full = (flags & RTW_FLAG_FULL_IMAGE) != 0;
  if (n_samples == 0) {  // nothing to add: nothing enqueued
    if (stats) *stats = rtw_stats{};
    return RTW_OK;
  }
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  if (stats)
    if (int e = copy_events(*c)) return e;
  const hipEvent_t e0 = stats ? c->ev[0] : nullptr, e1 = stats ? c->ev[1] : nullptr;
  const hipStream_t st = abi_stream(stream);
  int rc = enqueue_features(s->s, *c, f, sample_first, ts, d_albedo, d_normal, d_depth, st, e0, e1);
  if (rc == RTW_OK && stats) {
    rtw_stats out{};
    rc = collect_stats(*c, st, e0, e1, 0, &out);
    out.paths = out.rays;  // the samples the kernel traced, counted on the device
    out.total_ms = ms_since(t0);
    *stats = out;
  }
  return rc;
}

int rtw_render_features(rtw_scene* s, const rtw_camera* cam, const float bg[3], uint32_t w, uint32_t h, uint32_t spp,
                        uint64_t seed, float* albedo, float* normal, float* depth, rtw_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  const Frame f{cam, bg, w, h, spp, 1, seed};
  if (int e = check_features(s, f, albedo || normal || depth, 0)) return e;
  if (int e = check_sample_range(0, spp)) return e;
  DeviceCopy* c = need_copy(s->s, -1, nullptr);
  if (!c) return RTW_ENODEV;
  if (int e = check_image_max(w, h)) return e;
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  if (int e = copy_events(*c)) return e;
  const size_t px = (size_t)w * h;
  struct Buf {
    DevBuf& buf;
    float* host;
    size_t bytes;
  } bufs[3] = {{c->feat_albedo, albedo, px * 3 * sizeof(float)},
               {c->feat_normal, normal, px * 3 * sizeof(float)},
               {c->feat_depth, depth, px * 2 * sizeof(float)}};
  float* d[3] = {nullptr, nullptr, nullptr};
  for (int k = 0; k < 3; ++k) {
    if (!bufs[k].host) continue;
    if (int e = grow(bufs[k].buf, bufs[k].bytes)) return e;  // kept for the next frame, as rtw_render's image
    d[k] = static_cast<float*>(bufs[k].buf.p);
    HIPCHK(hipMemsetAsync(d[k], 0, bufs[k].bytes, nullptr), "hipMemsetAsync(features)");
  }
  const TileSet all{nullptr, 0, 1, (uint32_t)f.tiles()};
  rtw_stats st{};
  int rc = RTW_OK;
  if (spp) {
    rc = enqueue_features(s->s, *c, f, 0, all, d[0], d[1], d[2], nullptr, c->ev[0], c->ev[1]);
    if (rc == RTW_OK) rc = collect_stats(*c, nullptr, c->ev[0], c->ev[1], 0, &st);
    st.paths = st.rays;
  }
  for (int k = 0; k < 3 && rc == RTW_OK; ++k)
    if (d[k] && hipMemcpy(bufs[k].host, d[k], bufs[k].bytes, hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(RTW_ENODEV, "hipMemcpy(features)");
  st.total_ms = ms_since(t0);
  if (stats) *stats = st;
  return rc;
}

int rtw_render_ao_device(rtw_scene* s, int device, const rtw_camera* cam, uint32_t w, uint32_t h,
                         uint32_t sample_first, uint32_t n_samples, uint64_t seed, uint32_t ao_rays, float radius,
                         const uint32_t* d_tiles, uint32_t n_tiles, float* d_ao, void* stream, uint32_t flags,
                         rtw_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  const Frame f{cam, AO_NO_BG, w, h, n_samples, 1, seed};
  if (int e = check_features(s, f, d_ao, flags)) return e;
  if (int e = check_sample_range(sample_first, n_samples)) return e;
  if (int e = check_ao(ao_rays, radius)) return e;
  if (n_samples == 0) {  // nothing to add: nothing looked up, nothing enqueued
    if (stats) *stats = rtw_stats{};
    return RTW_OK;
  }
  DeviceCopy* c = need_copy(s->s, device);
  if (!c) return RTW_ENODEV;
  TileSet ts{d_tiles, 0, 1, d_tiles ? n_tiles : (uint32_t)f.tiles()};
  ts.full = (flags & RTW_FLAG_FULL_IMAGE) != 0;
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  if (stats)
    if (int e = copy_events(*c)) return e;
  const hipEvent_t e0 = stats ? c->ev[0] : nullptr, e1 = stats ? c->ev[1] : nullptr;
  const hipStream_t st = abi_stream(stream);
  int rc = enqueue_ao(s->s, *c, f, sample_first, ts, ao_rays, radius, d_ao, st, e0, e1);
  if (rc == RTW_OK && stats) {
    rtw_stats out{};
    rc = collect_stats(*c, st, e0, e1, 0, &out);
    ao_stats(out);
    out.total_ms = ms_since(t0);
    *stats = out;
  }
  return rc;
}

int rtw_render_ao(rtw_scene* s, const rtw_camera* cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                  uint32_t ao_rays, float radius, float* ao, rtw_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  const Frame f{cam, AO_NO_BG, w, h, spp, 1, seed};
  if (int e = check_features(s, f, ao, 0)) return e;
  if (int e = check_sample_range(0, spp)) return e;
  if (int e = check_ao(ao_rays, radius)) return e;
  DeviceCopy* c = need_copy(s->s, -1, nullptr);
  if (!c) return RTW_ENODEV;
  if (int e = check_image_max(w, h)) return e;
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  if (int e = copy_events(*c)) return e;
  const size_t bytes = (size_t)w * h * 2 * sizeof(float);
  if (int e = grow(c->ao_sums, bytes)) return e;  // kept for the next frame, as rtw_render's image
  float* d_ao = static_cast<float*>(c->ao_sums.p);
  HIPCHK(hipMemsetAsync(d_ao, 0, bytes, nullptr), "hipMemsetAsync(ao)");
  const TileSet all{nullptr, 0, 1, (uint32_t)f.tiles()};
  rtw_stats st{};
  int rc = RTW_OK;
  if (spp) {
    rc = enqueue_ao(s->s, *c, f, 0, all, ao_rays, radius, d_ao, nullptr, c->ev[0], c->ev[1]);
    if (rc == RTW_OK) rc = collect_stats(*c, nullptr, c->ev[0], c->ev[1], 0, &st);
    ao_stats(st);
  }
  if (rc == RTW_OK && hipMemcpy(ao, d_ao, bytes, hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(RTW_ENODEV, "hipMemcpy(ao)");
  st.total_ms = ms_since(t0);
  if (stats) *stats = st;
  return rc;
}

int rtw_sample_blocks(uint32_t sample_first, uint32_t n_samples, uint32_t* first, uint32_t* log2, uint32_t cap,
                      uint32_t* n_blocks) {
  if (!n_blocks || (cap && (!first || !log2))) return fail(RTW_EINVAL, "NULL argument");
  if (int e = check_sample_range(sample_first, n_samples)) return e;
  uint32_t firsts[SAMPLE_BLOCKS_MAX], log2s[SAMPLE_BLOCKS_MAX];
  const uint32_t nb = sample_blocks(sample_first, n_samples, firsts, log2s);
  *n_blocks = nb;
  if (cap < nb) return fail(RTW_EINVAL, "samples [%u, %u + %u) are %u blocks: cap %u", sample_first, sample_first,
                            n_samples, nb, cap);
  for (uint32_t k = 0; k < nb; ++k) {
    first[k] = firsts[k];
    log2[k] = log2s[k];
  }
  return RTW_OK;
}

int rtw_render_progressive(rtw_scene* s, const rtw_camera* cam, const float bg[3], uint32_t w, uint32_t h,
                           uint32_t spp, uint32_t max_depth, uint64_t seed, uint32_t step,
                           int (*sink)(const float* rgb_sum, const float* rgb_sq_sum, uint32_t w, uint32_t h,
                                       uint32_t samples_done, void* user),
                           void* user, rtw_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  const Frame f{cam, bg, w, h, spp, max_depth, seed};
  if (int e = check_frame(s, f, sink, true)) return e;
  if (int e = check_sample_range(0, spp)) return e;
  DeviceCopy* c = need_copy(s->s, -1, nullptr);
  if (!c) return RTW_ENODEV;
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  const size_t n = (size_t)w * h * 3, bytes = n * sizeof(float);
  if (int e = copy_events(*c)) return e;
  if (int e = grow(c->film_sum, bytes)) return e;  // kept for the next frame, as rtw_render's image
  if (int e = grow(c->film_sq, bytes)) return e;
  float* d_sum = static_cast<float*>(c->film_sum.p);
  float* d_sq = static_cast<float*>(c->film_sq.p);
  HIPCHK(hipMemsetAsync(d_sum, 0, bytes, nullptr), "hipMemsetAsync(sums)");
  HIPCHK(hipMemsetAsync(d_sq, 0, bytes, nullptr), "hipMemsetAsync(sums of squares)");
  std::vector<float> sum(n), sq(n);
  const TileSet all{nullptr, 0, 1, (uint32_t)f.tiles()};
  rtw_stats tot{};
  int rc = RTW_OK;
  for (uint32_t done = 0; rc == RTW_OK && done < spp;) {
    // 1, 2, 4, ... while the doubled count stays within `step` (0: always), then `step` more at a time; the frame's
    // last step ends at spp
    const uint64_t next = !done ? 1u : ((!step || 2ull * done <= step) ? 2ull * done : (uint64_t)done + step);
    const uint32_t end = (uint32_t)std::min<uint64_t>(next, spp);
    Frame chunk = f;
    chunk.spp = end - done;
    rc = enqueue_render_samples(s->s, *c, chunk, done, all, d_sum, d_sq, nullptr, 0, c->ev[0], c->ev[1]);
    rtw_stats st{};
    if (rc == RTW_OK) rc = collect_stats(*c, nullptr, c->ev[0], c->ev[1], 0, &st);
    if (rc == RTW_OK && (hipMemcpy(sum.data(), d_sum, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(sq.data(), d_sq, bytes, hipMemcpyDeviceToHost) != hipSuccess))
      rc = fail(RTW_ENODEV, "hipMemcpy(sums)");
    if (rc != RTW_OK) break;
    done = end;
    tot.rays += st.rays;
    tot.kernel_ms += st.kernel_ms;
    tot.paths = (uint64_t)w * h * done;
    if (int e = sink(sum.data(), sq.data(), w, h, done, user)) rc = e;
  }
  tot.total_ms = ms_since(t0);
  if (stats) *stats = tot;
  return rc;
}

int rtw_tonemap_device(int device, const float* d_rgb_sum, uint32_t n_pixels, uint32_t spp, uint8_t* d_rgb8,
                       void* stream) {
  if ((!d_rgb_sum || !d_rgb8) && n_pixels) return fail(RTW_EINVAL, "NULL buffer");
  if (spp == 0) return fail(RTW_EINVAL, "spp must be > 0");
  if (!n_pixels) return RTW_OK;
  DeviceGuard g;
  if (device >= 0) HIPCHK(hipSetDevice(device), "hipSetDevice");
  return enqueue_tonemap(d_rgb_sum, n_pixels, spp, d_rgb8, abi_stream(stream));
}

int rtw_tile_noise_device(int device, const float* d_sum, const float* d_sq, uint32_t w, uint32_t h,
                          const uint32_t* d_ids_in, uint32_t n_in, uint32_t samples, float threshold, float* d_err,
                          uint32_t* d_tile_samples, uint32_t* d_ids_out, uint32_t* d_n_out, void* stream) {
  if (!d_sum || !d_sq || !d_err || !d_ids_out || !d_n_out) return fail(RTW_EINVAL, "NULL buffer");
  if (int e = check_image_min(w, h)) return e;
  if (int e = check_image_max(w, h)) return e;
  if (samples == 0) return fail(RTW_EINVAL, "samples must be > 0");
  if (int e = check_threshold(threshold)) return e;
  DeviceGuard g;
  if (device >= 0) HIPCHK(hipSetDevice(device), "hipSetDevice");
  return enqueue_tile_noise(d_sum, d_sq, w, h, d_ids_in, n_in, samples, threshold, d_err, d_tile_samples, d_ids_out,
                            d_n_out, abi_stream(stream));
}

int rtw_render_adaptive_device(rtw_scene* s, int device, const rtw_camera* cam, const float bg[3], uint32_t w,
                               uint32_t h, uint32_t min_spp, uint32_t max_spp, uint32_t max_depth, uint64_t seed,
                               float threshold, float* d_sum, float* d_sq, uint32_t* d_tile_samples, float* d_tile_err,
                               void* stream, uint32_t flags, rtw_stats* stats) {
  const Frame f{cam, bg, w, h, max_spp, max_depth, seed};
  if (int e = check_frame(s, f, d_sum && d_sq && d_tile_samples, true)) return e;
  if (int e = check_adaptive(min_spp, max_spp, threshold)) return e;
  DeviceCopy* c = need_copy(s->s, device);
  if (!c) return RTW_ENODEV;
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  return render_adaptive(s->s, *c, f, min_spp, threshold, d_sum, d_sq, d_tile_samples, d_tile_err, abi_stream(stream),
                         flags, stats);
}

int rtw_render_adaptive(rtw_scene* s, const rtw_camera* cam, const float bg[3], uint32_t w, uint32_t h,
                        uint32_t min_spp, uint32_t max_spp, uint32_t max_depth, uint64_t seed, float threshold,
                        float* rgb_sum, float* rgb_sq_sum, uint32_t* tile_samples, float* tile_err, rtw_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  const Frame f{cam, bg, w, h, max_spp, max_depth, seed};
  if (int e = check_frame(s, f, rgb_sum && tile_samples, true)) return e;
  if (int e = check_adaptive(min_spp, max_spp, threshold)) return e;
  DeviceCopy* c = need_copy(s->s, -1, nullptr);
  if (!c) return RTW_ENODEV;
  if (int e = check_image_max(w, h)) return e;
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  const size_t bytes = (size_t)w * h * 3 * sizeof(float), nt = (size_t)f.tiles();
  if (int e = grow(c->film_sum, bytes)) return e;  // kept for the next frame, as rtw_render_progressive's
  if (int e = grow(c->film_sq, bytes)) return e;
  if (int e = grow(c->adapt_tiles, nt * (sizeof(uint32_t) + sizeof(float)))) return e;
  float* d_sum = static_cast<float*>(c->film_sum.p);
  float* d_sq = static_cast<float*>(c->film_sq.p);
  uint32_t* d_ts = static_cast<uint32_t*>(c->adapt_tiles.p);
  float* d_err = reinterpret_cast<float*>(d_ts + nt);
  rtw_stats st{};
  int rc = render_adaptive(s->s, *c, f, min_spp, threshold, d_sum, d_sq, d_ts, d_err, nullptr, 0, &st);
  if (rc == RTW_OK &&
      (hipMemcpy(rgb_sum, d_sum, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
       (rgb_sq_sum && hipMemcpy(rgb_sq_sum, d_sq, bytes, hipMemcpyDeviceToHost) != hipSuccess) ||
       hipMemcpy(tile_samples, d_ts, nt * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess ||
       (tile_err && hipMemcpy(tile_err, d_err, nt * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)))
    rc = fail(RTW_ENODEV, "hipMemcpy(adaptive frame)");
  st.total_ms = ms_since(t0);
  if (stats) *stats = st;
  return rc;
}

int rtw_tonemap_tiles_device(int device, const float* d_rgb_sum, uint32_t w, uint32_t h,
                             const uint32_t* d_tile_samples, uint8_t* d_rgb8, void* stream) {
  if (!d_rgb_sum || !d_tile_samples || !d_rgb8) return fail(RTW_EINVAL, "NULL buffer");
  if (int e = check_image_min(w, h)) return e;
  if (int e = check_image_max(w, h)) return e;
  DeviceGuard g;
  if (device >= 0) HIPCHK(hipSetDevice(device), "hipSetDevice");
  return enqueue_tonemap_tiles(d_rgb_sum, w, h, d_tile_samples, d_rgb8, abi_stream(stream));
}

int rtw_render_status(rtw_scene* s, int device) {
  if (!s) return fail(RTW_EINVAL, "NULL argument");
  DeviceCopy* c = need_copy(s->s, device);
  if (!c) return RTW_ENODEV;
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  HIPCHK(hipDeviceSynchronize(), "render (hipDeviceSynchronize)");
  return check_guard(*c);
}

// Test hook: overwrite the first two node4s of the device copy with a cycle (node 0 -> node 1 -> node 1
// ..., every box infinite, in both the 32-bit child words and the 16-bit codes), so that every ray's
// walk trips the traversal guard.  The host tables are untouched; renders of this copy are invalid.
int rtw_diag_corrupt_bvh(rtw_scene* s, int device) {
  if (!s) return fail(RTW_EINVAL, "NULL argument");
  if (!s->s.committed) return fail(RTW_ESTATE, "scene not committed");
  DeviceCopy* c = need_copy(s->s, device);
  if (!c) return RTW_ENODEV;
  if (c->scene.n_nodes < 2) return fail(RTW_EINVAL, "the scene's BVH has %u node4s (needs 2)", c->scene.n_nodes);
  DevNode4 nd[2];
  memset(nd, 0, sizeof nd);
  for (DevNode4& n : nd) {
    for (int k = 0; k < 4; ++k) {
      const float lo = k ? INFINITY : -1e30f, hi = k ? -INFINITY : 1e30f;  // slots 1-3 empty
      n.lo_x[k] = n.lo_y[k] = n.lo_z[k] = lo;
      n.hi_x[k] = n.hi_y[k] = n.hi_z[k] = hi;
    }
    n.child[0] = 1;
    n.code[0] = 1u;
  }
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  HIPCHK(hipMemcpy(const_cast<DevNode4*>(c->scene.nodes), nd, sizeof nd, hipMemcpyHostToDevice), "hipMemcpy(nodes)");
  if (c->scene.hnodes) {  // the half-precision table too: slot 0 = [-65504, +inf) on every axis, slots 1-3 empty
    DevNode4h hn[2];
    memset(hn, 0, sizeof hn);
    for (DevNode4h& n : hn) {
      for (uint16_t* ax : {&n.x[0][0], &n.y[0][0], &n.z[0][0]})
        for (int k = 0; k < 4; ++k) {
          const uint16_t lo = k ? 0x7C00 : 0x0000, hi = k ? 0xFC00 : 0x7C00;
          ax[k] = lo; ax[4 + k] = hi; ax[8 + k] = hi; ax[12 + k] = lo;
        }
      n.origin[0] = n.origin[1] = n.origin[2] = 0xFBFF;  // -65504
      n.code[0] = 1;
    }
    HIPCHK(hipMemcpy(const_cast<DevNode4h*>(c->scene.hnodes), hn, sizeof hn, hipMemcpyHostToDevice), "hipMemcpy(hnodes)");
  }
  return RTW_OK;
}

int rtw_render_stream(rtw_scene* s, const rtw_camera* cam, const float bg[3], uint32_t w, uint32_t h, uint32_t spp,
                      uint32_t max_depth, uint64_t seed, uint32_t band_rows, rtw_pixel_sink sink, void* user,
                      rtw_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  const Frame f{cam, bg, w, h, spp, max_depth, seed};
  if (int e = check_frame(s, f, sink)) return e;
  DeviceCopy* c = need_copy(s->s, -1, nullptr);
  if (!c) return RTW_ENODEV;
  const uint32_t tiles_x = f.tiles_x(), tiles_y = (h + 7u) / 8u;
  const uint32_t band_ty = std::max(1u, ((band_rows ? band_rows : 64u) + 7u) / 8u);  // tile rows per band
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  const size_t band_tiles = (size_t)band_ty * tiles_x;
  if (int e = grow(c->packed, band_tiles * 64 * 3 * sizeof(float))) return e;
  float* d_packed = static_cast<float*>(c->packed.p);
  if (int e = copy_events(*c)) return e;
  int rc = RTW_OK;
  std::vector<float> packed(band_tiles * 64 * 3);
  std::vector<rtw_pixel> px;
  rtw_stats tot{};
  for (uint32_t ty0 = 0; rc == RTW_OK && ty0 < tiles_y; ty0 += band_ty) {
    const uint32_t nty = std::min(band_ty, tiles_y - ty0), nt = nty * tiles_x;
    // tile row ty = output rows [8 ty, 8 ty + 8): the band's tiles are consecutive
    const TileSet band{nullptr, ty0 * tiles_x, 1, nt, true};
    rc = enqueue_render(s->s, *c, f, band, d_packed, nullptr, 0, c->ev[0], c->ev[1]);
    rtw_stats st{};
    if (rc == RTW_OK) rc = collect_stats(*c, nullptr, c->ev[0], c->ev[1], 0, &st);
    if (rc == RTW_OK && hipMemcpy(packed.data(), d_packed, (size_t)nt * 64 * 3 * sizeof(float),
                                  hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(RTW_ENODEV, "hipMemcpy(band)");
    if (rc != RTW_OK) break;
    tot.rays += st.rays;
    tot.kernel_ms += st.kernel_ms;
    // emit rows of this band in reference order: output row r <-> j = h-1-r, columns 0..w-1
    const uint32_t r0 = ty0 * 8u, r1 = std::min(h, (ty0 + nty) * 8u);
    px.clear();
    for (uint32_t r = r0; r < r1; ++r)
      for (uint32_t i = 0; i < w; ++i) {
        const size_t slot = (size_t)(r / 8u - ty0) * tiles_x + i / 8u, lane = (r % 8u) * 8u + (i % 8u);
        const float* v = &packed[(slot * 64 + lane) * 3];
        px.push_back(rtw_pixel{h - 1u - r, i, {v[0], v[1], v[2]}});
      }
    if (int e = sink(px.data(), (uint32_t)px.size(), user)) rc = e;
  }
  tot.paths = f.paths();
  tot.total_ms = ms_since(t0);
  if (stats) *stats = tot;
  return rc;
}

int rtw_path_kernel_times(rtw_scene* s, int device, float* ms, uint32_t max_n) {
  if (!s || (!ms && max_n)) return fail(RTW_EINVAL, "NULL argument");
  DeviceCopy* c = need_copy(s->s, device);
  if (!c) return RTW_ENODEV;
  DeviceGuard g;
  HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
  const uint32_t n = std::min(c->kev_count, max_n);
  int rc = (int)n;
  for (uint32_t q = 0; q < n; ++q) {  // the n most recent, oldest first
    const hipEvent_t* e = c->kev[(c->kev_head + 64u - n + q) % 64u];
    hipError_t err = hipEventSynchronize(e[1]);
    if (err == hipSuccess) err = hipEventElapsedTime(&ms[q], e[0], e[1]);
    if (err != hipSuccess) {
      rc = fail(RTW_ENODEV, "path-kernel events: %s", hipGetErrorString(err));
      break;
    }
  }
  c->kev_count = 0;
  if (rc >= 0 && n)  // the launches waited for: report a tripped traversal guard (its frame is invalid)
    if (int e = check_guard(*c)) rc = e;
  return rc;
}

int rtw_diag_recip(uint32_t n, const float* b, float* out) {
  if (n && (!b || !out)) return fail(RTW_EINVAL, "NULL argument");
  for (uint32_t k = 0; k < n; ++k) out[k] = recip_rn(b[k]);
  return RTW_OK;
}

int rtw_unpack_tiles_device(int device, uint32_t w, uint32_t h, const uint32_t* d_tiles, uint32_t n_tiles,
                            const float* d_packed, float* d_image, void* stream) {
  if (!d_tiles || !d_packed || !d_image) return fail(RTW_EINVAL, "NULL argument");
  DeviceGuard g;
  if (device >= 0) HIPCHK(hipSetDevice(device), "hipSetDevice");
  return enqueue_unpack(w, h, d_tiles, n_tiles, d_packed, d_image, abi_stream(stream));
}

}  // extern "C"
