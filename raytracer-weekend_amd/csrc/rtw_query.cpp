// rtw_query.cpp — the ten ray-query entry points of one device (rtw_hit_rays, rtw_occluded_rays, rtw_sample_rays,
// rtw_scatter_rays, rtw_camera_rays, each in a host form over host arrays and a device form over device arrays on the
// caller's stream) and their argument checks, on one shared runtime: Query opens the scene's device copy, stages the
// host forms' arrays chunk by chunk, and waits for and reports the device forms' statistics.  Plain HIP runtime API:
// the kernels and their launches are rtw_kernel.hip's (enqueue_hit_rays, enqueue_occluded_rays, enqueue_sample_rays,
// enqueue_scatter_rays, enqueue_camera_rays); the device copies, need_copy, the traversal guard's error word and the
// frame checks are rtw_render.cpp's.
//
// Every call checks in this order: a NULL argument (RTW_EINVAL), the scene's state (RTW_ESTATE; a flattened scene is
// asked for, so that a commit that found no device answers RTW_ENODEV), for the camera calls the frame, the path range
// and the shutter, then n == 0 (RTW_OK, zeroed stats, no array looked at and no device touched), the host scan of the
// records or the device arrays' alignment, and last the device copy (RTW_ENODEV).  A call that fails leaves *stats
// unwritten.
#include <algorithm>
#include <initializer_list>
#include <optional>

#include "../../include/rtw.h"
#include "rtw_scene.hpp"

namespace rtw {
namespace {

// What differs between the queries beyond their arrays.  Only hit_kernel, occluded_kernel and sample_kernel walk the
// BVH, so only their calls look at the traversal guard's error word (before anything is enqueued and after every wait)
// and count rays: a hit or occlusion query's are its n records, a radiance query's the segments its kernel counted on
// the device, as a render's.
struct Kind {
  const char* kernel;
  bool guard;    // check_guard before enqueueing and after waiting
  bool rays;     // stats->rays = n (else 0)
  bool counted;  // stats->rays = the device's segment counter (DeviceCopy::counters[0]), stats->paths = n
};
constexpr Kind HIT{"hit_kernel", true, true, false}, OCCLUDED{"occluded_kernel", true, true, false},
    SCATTER{"scatter_kernel", false, false, false}, CAMERA{"camera_rays_kernel", false, false, false},
    SAMPLE{"sample_kernel", true, false, true};

// One array of a host form: staged through `buf` in chunks, copied in from `in` and / or out to `out` (or NULL)
struct Staged {
  DevBuf& buf;
  const void* in;
  void* out;
  size_t elem;
  const char* what;
};

// One query call from entry to return
struct Query {
  const Kind& kind;
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  std::optional<DeviceGuard> restore;  // the caller's device, from open() to every return
  DeviceCopy* c = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;  // c's event pair, or NULL when the call times nothing
  rtw_stats st{};

  explicit Query(const Kind& k) : kind(k) {}

  // the scene's copy on `device` (-1: the first), its device made current
  int open(rtw_scene* s, int device, bool want_events) {
    c = need_copy(s->s, device, device < 0 ? nullptr : "");
    if (!c) return RTW_ENODEV;
    restore.emplace();
    HIPCHK(hipSetDevice(c->phys), "hipSetDevice");
    if (kind.guard)
      if (int e = check_guard(*c)) return e;
    if (want_events) {
      if (int e = copy_events(*c)) return e;
      e0 = c->ev[0];
      e1 = c->ev[1];
    }
    return RTW_OK;
  }

  // A host form's n records in chunks on the default stream: every array's chunk [k, k + m) copied in, enqueue(k, m)
  // between e0 and e1, copied out (which waits for the kernel); kernel_ms sums the chunks.  The host forms end here.
  template <class Enqueue>
  int run_staged(uint64_t n, rtw_stats* stats, std::initializer_list<Staged> arrays, Enqueue enqueue) {
    constexpr uint64_t CHUNK = 1ull << 20;
    for (const Staged& a : arrays)
      if (int e = grow(a.buf, std::min(n, CHUNK) * a.elem)) return e;
    for (uint64_t k = 0; k < n; k += CHUNK) {
      const uint64_t m = std::min(CHUNK, n - k);
      for (const Staged& a : arrays)
        if (const char* in = static_cast<const char*>(a.in))
          HIPCHK(hipMemcpy(a.buf.p, in + k * a.elem, m * a.elem, hipMemcpyHostToDevice), a.what);
      if (int e = enqueue(k, m)) return e;
      for (const Staged& a : arrays)
        if (char* out = static_cast<char*>(a.out))
          HIPCHK(hipMemcpy(out + k * a.elem, a.buf.p, m * a.elem, hipMemcpyDeviceToHost), a.what);
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
      st.kernel_ms += ms;
      if (kind.guard)
        if (int e = check_guard(*c)) return e;
      if (int e = count_segments()) return e;
    }
    return report(n, stats);
  }

  // a device form's end: nothing more without stats (no wait), else wait for the caller's stream
  int finish_device(hipStream_t stream, uint64_t n, rtw_stats* stats) {
    if (!stats) return RTW_OK;
    HIPCHK(hipStreamSynchronize(stream), kind.kernel);
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
    if (kind.guard)
      if (int e = check_guard(*c)) return e;
    st.kernel_ms = ms;
    if (int e = count_segments()) return e;
    return report(n, stats);
  }

  // after a wait: the segments the launches since enqueue_sample_rays' memset counted
  int count_segments() {
    if (!kind.counted) return RTW_OK;
    unsigned long long segments = 0;
    HIPCHK(hipMemcpy(&segments, c->counters, sizeof segments, hipMemcpyDeviceToHost), "hipMemcpy(counters)");
    st.rays += segments;
    return RTW_OK;
  }

  int report(uint64_t n, rtw_stats* stats) {
    if (kind.rays) st.rays = n;
    if (kind.counted) st.paths = n;
    st.total_ms = ms_since(t0);
    if (stats) *stats = st;
    return RTW_OK;
  }
};

int no_records(rtw_stats* stats) {
  if (stats) *stats = rtw_stats{};
  return RTW_OK;
}

// The checks every query call starts with, in the render calls' order; null_argument: one of the call's other pointers
// is NULL (the arrays only when n > 0: n == 0 looks at none)
int check_scene(const rtw_scene* s, bool null_argument) {
  if (!s || null_argument) return fail(RTW_EINVAL, "NULL argument");
  if (!s->s.flattened) return fail(RTW_ESTATE, "scene not committed");
  return RTW_OK;
}

// then the frame and the shutter as the render calls check them, and the path range.  Host only.
int camera_rays_check(const rtw_scene* s, const rtw_camera* cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t first,
                      uint64_t n, const void* rays) {
  if (int e = check_scene(s, !cam || (n && !rays))) return e;
  if (int e = check_image_min(w, h)) return e;
  if (int e = check_image_max(w, h)) return e;
  const uint64_t paths = (uint64_t)w * h * spp;  // < 2^64: w * h <= 2^32
  if (first > paths || n > paths - first)
    return fail(RTW_EINVAL, "paths [%llu, %llu + %llu) leave the frame's %llu", (unsigned long long)first,
                (unsigned long long)first, (unsigned long long)n, (unsigned long long)paths);
  if (int e = check_shutter(*cam, s->s.flat)) return e;
  // (a camera filled in by hand: the time draw's retry loop ends only for a non-empty range; camera.rs:72 panics)
  if (!(cam->time0 < cam->time1)) return fail(RTW_EINVAL, "camera shutter [%g, %g) is empty", cam->time0, cam->time1);
  return RTW_OK;
}

// the frame whose camera rays a call asks for (enqueue_camera_rays uses neither max_depth nor bg)
const float NO_BG[3] = {0.f, 0.f, 0.f};
Frame camera_frame(const rtw_camera* cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed) {
  return Frame{cam, NO_BG, w, h, spp, 0, seed};
}

}  // namespace
}  // namespace rtw

using namespace rtw;

extern "C" {

int rtw_hit_rays(rtw_scene* s, int device, uint64_t n, const void* rays, void* hits, rtw_stats* stats) {
  Query q(HIT);
  if (int e = check_scene(s, n && (!rays || !hits))) return e;
  if (n == 0) return no_records(stats);
  const rtw_ray* r = static_cast<const rtw_ray*>(rays);
  const float lo = s->s.flat.time_lo, hi = s->s.flat.time_hi;
  for (uint64_t k = 0; k < n; ++k)
    if (!(r[k].time >= lo && r[k].time <= hi))
      return fail(RTW_EINVAL, "ray %llu: time %g outside the committed motion range [%g, %g]", (unsigned long long)k,
                  r[k].time, lo, hi);
  if (int e = q.open(s, device, true)) return e;
  DeviceCopy& c = *q.c;
  const auto enqueue = [&](uint64_t, uint64_t m) {
    return enqueue_hit_rays(s->s, c, m, c.qrays.p, c.qhits.p, nullptr, q.e0, q.e1);
  };
  return q.run_staged(n, stats, {{c.qrays, rays, nullptr, sizeof(rtw_ray), "hipMemcpy(rays)"},
                                 {c.qhits, nullptr, hits, sizeof(rtw_hit), "hipMemcpy(hits)"}}, enqueue);
}

int rtw_hit_rays_device(rtw_scene* s, int device, uint64_t n, const void* d_rays, void* d_hits, void* stream,
                        rtw_stats* stats) {
  Query q(HIT);
  if (int e = check_scene(s, n && (!d_rays || !d_hits))) return e;
  if (n == 0) return no_records(stats);
  if (((uintptr_t)d_rays | (uintptr_t)d_hits) & 15u) return fail(RTW_EINVAL, "d_rays and d_hits must be 16-byte aligned");
  if (int e = q.open(s, device, stats != nullptr)) return e;
  const hipStream_t on = abi_stream(stream);
  if (int e = enqueue_hit_rays(s->s, *q.c, n, d_rays, d_hits, on, q.e0, q.e1)) return e;
  return q.finish_device(on, n, stats);
}

int rtw_occluded_rays(rtw_scene* s, int device, uint64_t n, const void* rays, const float* t_max, uint8_t* occluded,
                      rtw_stats* stats) {
  Query q(OCCLUDED);
  if (int e = check_scene(s, n && (!rays || !occluded))) return e;
  if (n == 0) return no_records(stats);
  const rtw_ray* r = static_cast<const rtw_ray*>(rays);
  const float lo = s->s.flat.time_lo, hi = s->s.flat.time_hi;
  for (uint64_t k = 0; k < n; ++k) {
    if (!(r[k].time >= lo && r[k].time <= hi))
      return fail(RTW_EINVAL, "ray %llu: time %g outside the committed motion range [%g, %g]", (unsigned long long)k,
                  r[k].time, lo, hi);
    if (t_max && t_max[k] != t_max[k]) return fail(RTW_EINVAL, "ray %llu: t_max is NaN", (unsigned long long)k);
  }
  if (int e = q.open(s, device, true)) return e;
  DeviceCopy& c = *q.c;
  const auto enqueue = [&](uint64_t, uint64_t m) {
    return enqueue_occluded_rays(s->s, c, m, c.qrays.p, t_max ? static_cast<const float*>(c.qtmax.p) : nullptr,
                                 static_cast<uint8_t*>(c.qoccluded.p), nullptr, q.e0, q.e1);
  };
  // (without bounds the qtmax entry has nothing to copy in and grows by nothing)
  return q.run_staged(n, stats, {{c.qrays, rays, nullptr, sizeof(rtw_ray), "hipMemcpy(rays)"},
                                 {c.qtmax, t_max, nullptr, t_max ? sizeof(float) : 0, "hipMemcpy(t_max)"},
                                 {c.qoccluded, nullptr, occluded, sizeof(uint8_t), "hipMemcpy(occluded)"}}, enqueue);
}

int rtw_occluded_rays_device(rtw_scene* s, int device, uint64_t n, const void* d_rays, const float* d_t_max,
                             uint8_t* d_occluded, void* stream, rtw_stats* stats) {
  Query q(OCCLUDED);
  if (int e = check_scene(s, n && (!d_rays || !d_occluded))) return e;
  if (n == 0) return no_records(stats);
  if ((uintptr_t)d_rays & 15u) return fail(RTW_EINVAL, "d_rays must be 16-byte aligned");
  if ((uintptr_t)d_t_max & 3u) return fail(RTW_EINVAL, "d_t_max must be 4-byte aligned");
  if (int e = q.open(s, device, stats != nullptr)) return e;
  const hipStream_t on = abi_stream(stream);
  if (int e = enqueue_occluded_rays(s->s, *q.c, n, d_rays, d_t_max, d_occluded, on, q.e0, q.e1)) return e;
  return q.finish_device(on, n, stats);
}

int rtw_sample_rays(rtw_scene* s, int device, uint64_t n, const void* rays, const float background[3],
                    uint32_t max_depth, void* samples, rtw_stats* stats) {
  Query q(SAMPLE);
  if (int e = check_scene(s, !background || (n && (!rays || !samples)))) return e;
  if (n == 0) return no_records(stats);
  const rtw_ray* r = static_cast<const rtw_ray*>(rays);
  const float lo = s->s.flat.time_lo, hi = s->s.flat.time_hi;
  for (uint64_t k = 0; k < n; ++k) {
    if (!(r[k].time >= lo && r[k].time <= hi))
      return fail(RTW_EINVAL, "ray %llu: time %g outside the committed motion range [%g, %g]", (unsigned long long)k,
                  r[k].time, lo, hi);
    if (r[k].stream == 0)
      return fail(RTW_EINVAL, "ray %llu: stream word 0 (the generator never leaves that state)", (unsigned long long)k);
  }
  if (int e = q.open(s, device, true)) return e;
  DeviceCopy& c = *q.c;
  const auto enqueue = [&](uint64_t, uint64_t m) {
    return enqueue_sample_rays(s->s, c, m, c.qrays.p, background, max_depth, c.qsamples.p, nullptr, q.e0, q.e1);
  };
  return q.run_staged(n, stats, {{c.qrays, rays, nullptr, sizeof(rtw_ray), "hipMemcpy(rays)"},
                                 {c.qsamples, nullptr, samples, sizeof(rtw_sample), "hipMemcpy(samples)"}}, enqueue);
}

int rtw_sample_rays_device(rtw_scene* s, int device, uint64_t n, const void* d_rays, const float background[3],
                           uint32_t max_depth, void* d_samples, void* stream, rtw_stats* stats) {
  Query q(SAMPLE);
  if (int e = check_scene(s, !background || (n && (!d_rays || !d_samples)))) return e;
  if (n == 0) return no_records(stats);
  if (((uintptr_t)d_rays | (uintptr_t)d_samples) & 15u)
    return fail(RTW_EINVAL, "d_rays and d_samples must be 16-byte aligned");
  if (int e = q.open(s, device, stats != nullptr)) return e;
  const hipStream_t on = abi_stream(stream);
  if (int e = enqueue_sample_rays(s->s, *q.c, n, d_rays, background, max_depth, d_samples, on, q.e0, q.e1)) return e;
  return q.finish_device(on, n, stats);
}

int rtw_scatter_rays(rtw_scene* s, int device, uint64_t n, const void* rays, const void* hits,
                     const float background[3], void* out_rays, void* out_scatter, rtw_stats* stats) {
  Query q(SCATTER);
  if (int e = check_scene(s, !background || (n && (!rays || !hits || !out_rays || !out_scatter)))) return e;
  if (n == 0) return no_records(stats);
  const rtw_ray* r = static_cast<const rtw_ray*>(rays);
  for (uint64_t k = 0; k < n; ++k)
    if (r[k].stream == 0)
      return fail(RTW_EINVAL, "record %llu: stream word 0 (the generator never leaves that state)",
                  (unsigned long long)k);
  if (int e = q.open(s, device, true)) return e;
  DeviceCopy& c = *q.c;
  // in place on the device: the staged rays become the scattered rays
  const auto enqueue = [&](uint64_t, uint64_t m) {
    return enqueue_scatter_rays(s->s, c, m, c.qrays.p, c.qhits.p, background, c.qrays.p, c.qscatter.p, nullptr, q.e0,
                                q.e1);
  };
  return q.run_staged(n, stats, {{c.qrays, rays, out_rays, sizeof(rtw_ray), "hipMemcpy(rays)"},
                                 {c.qhits, hits, nullptr, sizeof(rtw_hit), "hipMemcpy(hits)"},
                                 {c.qscatter, nullptr, out_scatter, sizeof(rtw_scatter), "hipMemcpy(scatter)"}},
                      enqueue);
}

int rtw_scatter_rays_device(rtw_scene* s, int device, uint64_t n, const void* d_rays, const void* d_hits,
                            const float background[3], void* d_out_rays, void* d_out_scatter, void* stream,
                            rtw_stats* stats) {
  Query q(SCATTER);
  if (int e = check_scene(s, !background || (n && (!d_rays || !d_hits || !d_out_rays || !d_out_scatter)))) return e;
  if (n == 0) return no_records(stats);
  if (((uintptr_t)d_rays | (uintptr_t)d_hits | (uintptr_t)d_out_rays | (uintptr_t)d_out_scatter) & 15u)
    return fail(RTW_EINVAL, "d_rays, d_hits, d_out_rays and d_out_scatter must be 16-byte aligned");
  if (int e = q.open(s, device, stats != nullptr)) return e;
  const hipStream_t on = abi_stream(stream);
  if (int e = enqueue_scatter_rays(s->s, *q.c, n, d_rays, d_hits, background, d_out_rays, d_out_scatter, on, q.e0, q.e1))
    return e;
  return q.finish_device(on, n, stats);
}

int rtw_camera_rays(rtw_scene* s, int device, const rtw_camera* cam, uint32_t w, uint32_t h, uint32_t spp,
                    uint64_t seed, uint64_t first, uint64_t n, void* rays, rtw_stats* stats) {
  Query q(CAMERA);
  if (int e = camera_rays_check(s, cam, w, h, spp, first, n, rays)) return e;
  if (n == 0) return no_records(stats);
  if (int e = q.open(s, device, true)) return e;
  DeviceCopy& c = *q.c;
  const Frame f = camera_frame(cam, w, h, spp, seed);
  const auto enqueue = [&](uint64_t k, uint64_t m) {
    return enqueue_camera_rays(c, f, first + k, m, c.qrays.p, nullptr, q.e0, q.e1);
  };
  return q.run_staged(n, stats, {{c.qrays, nullptr, rays, sizeof(rtw_ray), "hipMemcpy(rays)"}}, enqueue);
}

int rtw_camera_rays_device(rtw_scene* s, int device, const rtw_camera* cam, uint32_t w, uint32_t h, uint32_t spp,
                           uint64_t seed, uint64_t first, uint64_t n, void* d_rays, void* stream, rtw_stats* stats) {
  Query q(CAMERA);
  if (int e = camera_rays_check(s, cam, w, h, spp, first, n, d_rays)) return e;
  if (n == 0) return no_records(stats);
  if ((uintptr_t)d_rays & 15u) return fail(RTW_EINVAL, "d_rays must be 16-byte aligned");
  if (int e = q.open(s, device, stats != nullptr)) return e;
  const hipStream_t on = abi_stream(stream);
  if (int e = enqueue_camera_rays(*q.c, camera_frame(cam, w, h, spp, seed), first, n, d_rays, on, q.e0, q.e1)) return e;
  return q.finish_device(on, n, stats);
}

}  // extern "C"
