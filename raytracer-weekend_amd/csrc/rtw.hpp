// rtw.hpp — C++ mirror of raytracer_weekend_lib's public API on top of the C-ABI.
//
// Same names and argument meaning as the Rust crate, so host code reads like
// console_app: build a world, then Raytracer(world, cam, background, w, h, spp).render().
//   Rust                                          C++ (this header)
//   Camera::new(from, at, up, vfov, a, ap, f, t0, t1)   Camera::new_(...)       camera.rs:25-64
//   SolidColor::new_rgb / Checker::new / UVDebug::new   world.solid_rgb / checker / uv_debug
//   Lambertian::new / Metal::new / Dielectric::new /    world.lambertian / metal / dielectric /
//   DiffuseLight::new                                   diffuse_light                material.rs, light_source.rs
//   Sphere::new / MovingSphere::new / XYRectangle::new  world.sphere / moving_sphere / xy_rect ...
//   Cuboid::new(...).rotate_y(a).translate(v)           world.translate(v, [&]{ world.rotate_y(a, [&]{ world.cuboid(...); }); })
//   BvhNode::new(objs, t0, t1, rng)                     world.bvh(t0, t1, [&]{ ... })
//   load_wavefront_obj(path, rng)                       world.load_wavefront_obj(path)
//   Raytracer::new(..).render() -> Pixel stream         Raytracer(..).render() -> std::vector<Pixel>
//   world.hit(&ray, 0.001, INFINITY) -> Option<HitRecord>  world.hit_rays(rays) -> std::vector<Hit>  hittable/mod.rs:22-69
//   world.hit(&ray, 0.001, t_max).is_some()              world.occluded_rays(rays, t_max) -> std::vector<uint8_t>
//   cam.get_ray(u, v, rng) per path of a frame         world.camera_rays(cam, w, h, spp, seed) -> std::vector<Ray>  camera.rs:66-74
//   rec.material.scatter(&ray, &rec, rng) / emitted()   world.scatter_rays(rays, hits, background) -> {rays, Scatter}  material.rs:23-26
//   raytracer.sample_ray(&ray, rng, depth) -> Color      world.sample_rays(rays, background, max_depth) -> std::vector<Sample>  lib.rs:97-117
//   (no counterpart: the frame in growing steps)        Raytracer(..).render_progressive(on_frame, step); sample_blocks; tonemap_device
//   (no counterpart: a sample count per 8x8 tile)       Raytracer(..).render_adaptive(threshold, min_spp) -> AdaptiveFrame; tile_noise_device; tonemap_tiles
//   (no counterpart: a denoiser's guides)               Raytracer(..).render_features() -> FeatureFrame; render_features_device
//   (no counterpart: ambient occlusion)                 Raytracer(..).render_ao(ao_rays, radius); render_ao_device
//   (no counterpart: the denoiser)                       denoise_device; denoise; denoise_scratch_bytes
//   (no counterpart: temporal accumulation)              temporal_device; temporal; denoise_counts_device; denoise_counts
// Errors (the reference panics) throw rtw::Error with rtw_last_error()'s message.
#pragma once
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rtw.h"

namespace rtw {

struct Error : std::runtime_error {
  int code;
  Error(int c, const char* m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) {
  if (rc != RTW_OK) throw Error(rc, rtw_last_error());
}

struct Vec3 {
  float x, y, z;
};
using Point3 = Vec3;
using Color = Vec3;

// lib.rs:120-126: row counts from the bottom (j), colour is the un-normalised sum.
struct Pixel {
  uint32_t row, column;
  Color color;
};

using TextureId = uint32_t;
using MaterialId = uint32_t;

// ray.rs Ray (+ the segment's stream word, which keys a ConstantMedium's free path) and hittable/mod.rs:22-29
// HitRecord, laid out as the C-ABI's rtw_ray / rtw_hit
struct Ray {
  Point3 origin;
  Vec3 direction;
  float time = 0.f;
  uint32_t reserved = 0;
  uint64_t stream = 0;
};
struct Hit {
  Point3 p;
  Vec3 normal;
  float t, u, v;
  MaterialId material;
  uint32_t key, flags;
  bool hit() const { return flags & RTW_HIT_HIT; }
  bool front_face() const { return flags & RTW_HIT_FRONT_FACE; }
};
static_assert(sizeof(Ray) == sizeof(rtw_ray) && sizeof(Hit) == sizeof(rtw_hit), "rtw::Ray / rtw::Hit mirror rtw.h");
// material.rs:18-21 Scatter + Material::emitted: one step of sample_ray after world.hit, laid out as rtw_scatter
struct Scatter {
  Color attenuation, emitted;
  uint32_t flags, reserved;
  bool scattered() const { return flags & RTW_SCATTER_SCATTERED; }
  bool miss() const { return flags & RTW_SCATTER_MISS; }
  bool bad() const { return flags & RTW_SCATTER_BAD; }
};
static_assert(sizeof(Scatter) == sizeof(rtw_scatter), "rtw::Scatter mirrors rtw.h");
// lib.rs:97-117 sample_ray's value for a caller's ray, laid out as rtw_sample
struct Sample {
  Color color;
  uint32_t segments;
  uint64_t stream;
  uint32_t flags, reserved;
  bool missed() const { return flags & RTW_SAMPLE_END_MISS; }
  bool no_scatter() const { return flags & RTW_SAMPLE_END_NO_SCATTER; }
  bool depth_exhausted() const { return flags & RTW_SAMPLE_END_DEPTH; }
  bool bad() const { return flags & RTW_SAMPLE_BAD_RAY; }
};
static_assert(sizeof(Sample) == sizeof(rtw_sample), "rtw::Sample mirrors rtw.h");

struct Camera {
  rtw_camera c{};
  static Camera new_(Point3 from, Point3 at, Vec3 up, float vfov, float aspect, float aperture, float focus,
                     float t0, float t1) {
    Camera k;
    const float f[3] = {from.x, from.y, from.z}, a[3] = {at.x, at.y, at.z}, u[3] = {up.x, up.y, up.z};
    check(rtw_camera_new(f, a, u, vfov, aspect, aperture, focus, t0, t1, &k.c));
    return k;
  }
};

class World {
 public:
  World() { check(rtw_scene_create(&s_)); }
  ~World() { rtw_scene_destroy(s_); }
  World(const World&) = delete;
  World& operator=(const World&) = delete;
  rtw_scene* raw() const { return s_; }

  TextureId solid_rgb(float r, float g, float b) { TextureId t; check(rtw_texture_solid(s_, r, g, b, &t)); return t; }
  TextureId checker(TextureId odd, TextureId even, float freq) { TextureId t; check(rtw_texture_checker(s_, odd, even, freq, &t)); return t; }
  TextureId image(const uint8_t* rgb, uint32_t w, uint32_t h) { TextureId t; check(rtw_texture_image(s_, rgb, w, h, &t)); return t; }
  TextureId uv_debug() { TextureId t; check(rtw_texture_uvdebug(s_, &t)); return t; }
  // Noise::new(Perlin::new(rng), scale): Perlin tables from the build's seeded stream
  TextureId noise(float scale, uint64_t perlin_seed) {
    float g[768];
    uint32_t p[768];
    check(rtw_perlin_generate(perlin_seed, g, p));
    TextureId t;
    check(rtw_texture_noise(s_, g, p, scale, &t));
    return t;
  }

  MaterialId lambertian(TextureId t) { MaterialId m; check(rtw_material_lambertian(s_, t, &m)); return m; }
  MaterialId lambertian_solid(Color c) { return lambertian(solid_rgb(c.x, c.y, c.z)); }
  MaterialId metal(Color albedo, float fuzz) { MaterialId m; check(rtw_material_metal(s_, albedo.x, albedo.y, albedo.z, fuzz, &m)); return m; }
  MaterialId dielectric(float ir) { MaterialId m; check(rtw_material_dielectric(s_, ir, &m)); return m; }
  MaterialId diffuse_light(TextureId t) { MaterialId m; check(rtw_material_diffuse_light(s_, t, &m)); return m; }
  MaterialId isotropic(TextureId t) { MaterialId m; check(rtw_material_isotropic(s_, t, &m)); return m; }

  void sphere(Point3 c, float r, MaterialId m) { check(rtw_add_spheres(s_, 1, &c.x, &c.y, &c.z, &r, &m)); }
  void moving_sphere(Point3 c0, float t0, Point3 c1, float t1, float r, MaterialId m) {
    check(rtw_add_moving_spheres(s_, 1, &c0.x, &c0.y, &c0.z, &t0, &c1.x, &c1.y, &c1.z, &t1, &r, &m));
  }
  void rect(uint32_t axis, float a0, float a1, float b0, float b1, float k, MaterialId m) {
    check(rtw_add_rects(s_, 1, &axis, &a0, &a1, &b0, &b1, &k, &m));
  }
  void xy_rect(float x0, float x1, float y0, float y1, float k, MaterialId m) { rect(0, x0, x1, y0, y1, k, m); }
  void xz_rect(float x0, float x1, float z0, float z1, float k, MaterialId m) { rect(1, x0, x1, z0, z1, k, m); }
  void yz_rect(float y0, float y1, float z0, float z1, float k, MaterialId m) { rect(2, y0, y1, z0, z1, k, m); }
  void cuboid(Point3 p0, Point3 p1, MaterialId m) {
    const float a[3] = {p0.x, p0.y, p0.z}, b[3] = {p1.x, p1.y, p1.z};
    check(rtw_add_cuboid(s_, a, b, m));
  }
  void triangle(const Point3 v[3], MaterialId m) {  // Triangle::new_flat_shaded
    const float f[9] = {v[0].x, v[0].y, v[0].z, v[1].x, v[1].y, v[1].z, v[2].x, v[2].y, v[2].z};
    check(rtw_add_triangles(s_, 1, f, nullptr, nullptr, nullptr, nullptr, m));
  }
  uint32_t load_wavefront_obj(const std::string& path, uint32_t material_override = UINT32_MAX) {
    uint32_t n = 0;
    check(rtw_load_wavefront_obj(s_, path.c_str(), nullptr, material_override, &n));
    return n;
  }
  template <class F> void list(F&& body) { check(rtw_begin_list(s_)); body(); check(rtw_end(s_)); }
  template <class F> void bvh(float t0, float t1, F&& body) { check(rtw_begin_bvh(s_, t0, t1)); body(); check(rtw_end(s_)); }
  template <class F> void translate(Vec3 off, F&& body) { check(rtw_begin_translate(s_, off.x, off.y, off.z)); body(); check(rtw_end(s_)); }
  template <class F> void rotate_y(float deg, F&& body) { check(rtw_begin_rotate_y(s_, deg)); body(); check(rtw_end(s_)); }
  // ConstantMedium::new(boundary, density, texture): body adds the boundary
  template <class F> void constant_medium(float density, TextureId t, F&& body) {
    check(rtw_begin_constant_medium(s_, density, t, nullptr)); body(); check(rtw_end(s_));
  }

  // console_app/src/scenes.rs presets; returns the camera and background
  void preset(const std::string& name, float aspect, uint64_t seed, const std::string& models, Camera& cam, Color& bg) {
    float b[3];
    check(rtw_scene_preset(s_, name.c_str(), aspect, seed, models.c_str(), &cam.c, b));
    bg = Color{b[0], b[1], b[2]};
  }
  // every camera of a preset (animated-book2-final-scene has 30, scenes.rs:622-667)
  static std::vector<Camera> preset_cameras(const std::string& name, float aspect, const std::string& models) {
    uint32_t n = 0;
    check(rtw_preset_cameras(name.c_str(), aspect, models.c_str(), nullptr, 0, &n));
    std::vector<rtw_camera> raw(n);
    check(rtw_preset_cameras(name.c_str(), aspect, models.c_str(), raw.data(), n, &n));
    std::vector<Camera> out(n);
    for (uint32_t k = 0; k < n; ++k) out[k].c = raw[k];
    return out;
  }
  void commit(int device = -1) { check(rtw_scene_commit(s_, device)); }
  // [Box<dyn Hittable>]::hit(&ray, 0.001, INFINITY) for every ray (hittable/mod.rs:57-69), on the GPU; blocking
  std::vector<Hit> hit_rays(const std::vector<Ray>& rays, int device = -1, rtw_stats* st = nullptr) const {
    std::vector<Hit> hits(rays.size());
    check(rtw_hit_rays(s_, device, rays.size(), rays.data(), hits.data(), st));
    return hits;
  }
  // world.hit(&ray, 0.001, t_max[k]).is_some() for every ray, on the GPU; blocking.  t_max empty: +inf for every ray;
  // else one bound per ray (inclusive).  -> 0 = free, RTW_OCCLUDED_HIT
  std::vector<uint8_t> occluded_rays(const std::vector<Ray>& rays, const std::vector<float>& t_max = {},
                                     int device = -1, rtw_stats* st = nullptr) const {
    if (!t_max.empty() && t_max.size() != rays.size()) throw Error(RTW_EINVAL, "rays and t_max differ in length");
    std::vector<uint8_t> occ(rays.size());
    check(rtw_occluded_rays(s_, device, rays.size(), rays.data(), t_max.empty() ? nullptr : t_max.data(), occ.data(),
                            st));
    return occ;
  }
  // the render's camera rays of paths [first, first + n) of a w x h x spp frame, in rtw_render's output order
  // (lib.rs:84-86, camera.rs:66-74); n = UINT64_MAX: to the frame's end
  std::vector<Ray> camera_rays(const Camera& cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                               uint64_t first = 0, uint64_t n = UINT64_MAX, int device = -1,
                               rtw_stats* st = nullptr) const {
    const uint64_t paths = (uint64_t)w * h * spp;
    if (n == UINT64_MAX) n = first <= paths ? paths - first : 0;
    std::vector<Ray> rays(n);
    check(rtw_camera_rays(s_, device, &cam.c, w, h, spp, seed, first, n, rays.data(), st));
    return rays;
  }
  // diagnostics: the per-tile lists a render of (cam, w x h) builds for its camera rays (rtw_diag_tile_lists): 8 words
  // per 8x8 tile, in tile order; *n_over (or nullptr) = the tiles on overflow
  std::vector<uint32_t> tile_lists(const Camera& cam, uint32_t w, uint32_t h, int device = -1,
                                   uint32_t* n_over = nullptr) const {
    std::vector<uint32_t> rec((size_t)((w + 7u) / 8u) * ((h + 7u) / 8u) * 8u);
    const int n = rtw_diag_tile_lists(s_, device, &cam.c, w, h, rec.data(), rec.size(), n_over, nullptr, 0);
    if (n < 0) check(n);
    return rec;
  }
  // Material::scatter + emitted for every (ray, hit record) pair (lib.rs:102-116): the scattered rays replace `rays`
  std::vector<Scatter> scatter_rays(std::vector<Ray>& rays, const std::vector<Hit>& hits, Color background,
                                    int device = -1, rtw_stats* st = nullptr) const {
    if (rays.size() != hits.size()) throw Error(RTW_EINVAL, "rays and hits differ in length");
    std::vector<Scatter> sc(rays.size());
    const float bg[3] = {background.x, background.y, background.z};
    check(rtw_scatter_rays(s_, device, rays.size(), rays.data(), hits.data(), bg, rays.data(), sc.data(), st));
    return sc;
  }
  // Raytracer::sample_ray for every ray (lib.rs:97-117), each whole path on the GPU in one launch; a ray's stream
  // word (non-zero) seeds its path's draws; blocking
  std::vector<Sample> sample_rays(const std::vector<Ray>& rays, Color background, uint32_t max_depth = 50,
                                  int device = -1, rtw_stats* st = nullptr) const {
    std::vector<Sample> out(rays.size());
    const float bg[3] = {background.x, background.y, background.z};
    check(rtw_sample_rays(s_, device, rays.size(), rays.data(), bg, max_depth, out.data(), st));
    return out;
  }

 private:
  rtw_scene* s_ = nullptr;
};

// Raytracer::render_adaptive's frame: flat RGB sums in render_sums' layout, and per 8x8 tile (row-major, ragged edges
// whole) the samples its pixels hold and its last noise estimate
struct AdaptiveFrame {
  std::vector<float> sums;
  std::vector<uint32_t> tile_samples;
  std::vector<float> tile_err;
};

// Raytracer::render_features' frame: per pixel, in render_sums' order, the sums over its camera rays of the first hit's
// albedo (3 floats), normal (3) and depth (2: t and the hit count)
struct FeatureFrame {
  std::vector<float> albedo, normal, depth;
};

// lib.rs:40-95
class Raytracer {
 public:
  Raytracer(World& world, const Camera& cam, Color background, uint32_t w, uint32_t h, uint32_t spp,
            uint64_t seed = 0, uint32_t max_depth = 50)
      : world_(world), cam_(cam), bg_(background), w_(w), h_(h), spp_(spp), seed_(seed), depth_(max_depth) {}

  // Un-normalised per-pixel sums, flat RGB in the reference emission order (lib.rs:58).
  std::vector<float> render_sums(rtw_stats* st = nullptr) const {
    std::vector<float> out((size_t)w_ * h_ * 3);
    const float bg[3] = {bg_.x, bg_.y, bg_.z};
    check(rtw_render(world_.raw(), &cam_.c, bg, w_, h_, spp_, depth_, seed_, out.data(), st));
    return out;
  }
  // Raytracer::render(): Pixel stream, rows h-1..0, columns 0..w-1
  std::vector<Pixel> render(rtw_stats* st = nullptr) const {
    std::vector<float> s = render_sums(st);
    std::vector<Pixel> px;
    px.reserve((size_t)w_ * h_);
    for (uint32_t r = 0; r < h_; ++r)
      for (uint32_t i = 0; i < w_; ++i) {
        const float* c = &s[((size_t)r * w_ + i) * 3];
        px.push_back(Pixel{h_ - 1 - r, i, Color{c[0], c[1], c[2]}});
      }
    return px;
  }
  // The frame in growing steps (rtw_render_progressive): on_frame(sums, sums of squares, samples done) -> int after
  // each, flat RGB in render_sums' layout; a non-zero return stops the render and comes back as the result.
  template <class F> int render_progressive(F&& on_frame, uint32_t step = 0, rtw_stats* st = nullptr) const {
    const float bg[3] = {bg_.x, bg_.y, bg_.z};
    auto* fn = &on_frame;
    using Fn = typename std::remove_reference<F>::type;
    const rtw_frame_sink sink = [](const float* sum, const float* sq, uint32_t, uint32_t, uint32_t done, void* user) {
      return (int)(*static_cast<Fn*>(user))(sum, sq, done);
    };
    const int rc = rtw_render_progressive(world_.raw(), &cam_.c, bg, w_, h_, spp_, depth_, seed_, step, sink,
                                          const_cast<void*>(static_cast<const void*>(fn)), st);
    if (rc < 0) check(rc);
    return rc;
  }
  // Samples [first, first + n) of the tile set added onto the device sums d_sum and d_sq (or nullptr)
  // (rtw_render_samples_device; the constructor's spp is not used); d_tile_ids = nullptr: the whole image
  void render_samples_device(int device, uint32_t first, uint32_t n, float* d_sum, float* d_sq,
                             const uint32_t* d_tile_ids = nullptr, uint32_t n_tiles = 0, void* stream = nullptr,
                             uint32_t flags = 0, rtw_stats* st = nullptr) const {
    const float bg[3] = {bg_.x, bg_.y, bg_.z};
    check(rtw_render_samples_device(world_.raw(), device, &cam_.c, bg, w_, h_, first, n, depth_, seed_, d_tile_ids,
                                    n_tiles, d_sum, d_sq, stream, flags, st));
  }
  // The frame with a sample count per tile (rtw_render_adaptive; the constructor's spp is the maximum): a tile stops at
  // the first of min_spp, 2 min_spp, ... samples at which its noise estimate is <= threshold, and then holds
  // render_sums' pixels of a frame of that many samples.
  AdaptiveFrame render_adaptive(float threshold, uint32_t min_spp = 16, rtw_stats* st = nullptr) const {
    const size_t tiles = (size_t)((w_ + 7u) / 8u) * ((h_ + 7u) / 8u);
    AdaptiveFrame f{std::vector<float>((size_t)w_ * h_ * 3), std::vector<uint32_t>(tiles), std::vector<float>(tiles)};
    const float bg[3] = {bg_.x, bg_.y, bg_.z};
    check(rtw_render_adaptive(world_.raw(), &cam_.c, bg, w_, h_, min_spp, spp_, depth_, seed_, threshold, f.sums.data(),
                              nullptr, f.tile_samples.data(), f.tile_err.data(), st));
    return f;
  }
  // The same into device memory (rtw_render_adaptive_device; blocking on `stream`): full-layout d_sum and d_sq, zeroed
  // by the call, d_tile_samples[tiles] and d_tile_err[tiles] (or nullptr)
  void render_adaptive_device(int device, float threshold, uint32_t min_spp, float* d_sum, float* d_sq,
                              uint32_t* d_tile_samples, float* d_tile_err = nullptr, void* stream = nullptr,
                              uint32_t flags = 0, rtw_stats* st = nullptr) const {
    const float bg[3] = {bg_.x, bg_.y, bg_.z};
    check(rtw_render_adaptive_device(world_.raw(), device, &cam_.c, bg, w_, h_, min_spp, spp_, depth_, seed_, threshold,
                                     d_sum, d_sq, d_tile_samples, d_tile_err, stream, flags, st));
  }
  // The denoiser's guides for this frame (rtw_render_features): first-hit albedo, normal and depth summed over each
  // pixel's spp camera rays (the background, +0 and (0, 0) for a miss); sample s is render_sums' camera ray s
  FeatureFrame render_features(rtw_stats* st = nullptr) const {
    const size_t px = (size_t)w_ * h_;
    FeatureFrame f{std::vector<float>(px * 3), std::vector<float>(px * 3), std::vector<float>(px * 2)};
    const float bg[3] = {bg_.x, bg_.y, bg_.z};
    check(rtw_render_features(world_.raw(), &cam_.c, bg, w_, h_, spp_, seed_, f.albedo.data(), f.normal.data(),
                              f.depth.data(), st));
    return f;
  }
  // Samples [first, first + n) of the tile set as features added onto the device sums d_albedo, d_normal (3 floats per
  // pixel) and d_depth (2), each or nullptr, not all (rtw_render_features_device; the constructor's spp is not used);
  // tiles, layouts and flags as render_samples_device
  void render_features_device(int device, uint32_t first, uint32_t n, float* d_albedo, float* d_normal, float* d_depth,
                              const uint32_t* d_tile_ids = nullptr, uint32_t n_tiles = 0, void* stream = nullptr,
                              uint32_t flags = 0, rtw_stats* st = nullptr) const {
    const float bg[3] = {bg_.x, bg_.y, bg_.z};
    check(rtw_render_features_device(world_.raw(), device, &cam_.c, bg, w_, h_, first, n, seed_, d_tile_ids, n_tiles,
                                     d_albedo, d_normal, d_depth, stream, flags, st));
  }
  // The ambient-occlusion buffer of this frame (rtw_render_ao): per pixel, in render_sums' order, the sums over its spp
  // camera rays of (open, cast) -- of the ao_rays rays cast from each first hit, those unoccluded up to `radius`
  // (INFINITY: sky visibility), and those cast; mean AO = open / cast
  std::vector<float> render_ao(uint32_t ao_rays, float radius, rtw_stats* st = nullptr) const {
    std::vector<float> ao((size_t)w_ * h_ * 2);
    check(rtw_render_ao(world_.raw(), &cam_.c, w_, h_, spp_, seed_, ao_rays, radius, ao.data(), st));
    return ao;
  }
  // Samples [first, first + n) of the tile set as ambient occlusion added onto the device sums d_ao (2 floats per
  // pixel) (rtw_render_ao_device; the constructor's spp is not used); tiles, layouts and flags as
  // render_features_device
  void render_ao_device(int device, uint32_t first, uint32_t n, uint32_t ao_rays, float radius, float* d_ao,
                        const uint32_t* d_tile_ids = nullptr, uint32_t n_tiles = 0, void* stream = nullptr,
                        uint32_t flags = 0, rtw_stats* st = nullptr) const {
    check(rtw_render_ao_device(world_.raw(), device, &cam_.c, w_, h_, first, n, seed_, ao_rays, radius, d_tile_ids,
                               n_tiles, d_ao, stream, flags, st));
  }

 private:
  World& world_;
  Camera cam_;
  Color bg_;
  uint32_t w_, h_, spp_;
  uint64_t seed_;
  uint32_t depth_;
};

// the aligned power-of-two blocks (first, log2 of the size) samples [first, first + n) run as (rtw_sample_blocks)
inline std::vector<std::pair<uint32_t, uint32_t>> sample_blocks(uint32_t first, uint32_t n) {
  uint32_t f[62], l[62], nb = 0;
  check(rtw_sample_blocks(first, n, f, l, 62, &nb));
  std::vector<std::pair<uint32_t, uint32_t>> out(nb);
  for (uint32_t k = 0; k < nb; ++k) out[k] = {f[k], l[k]};
  return out;
}
// rtw_tonemap over device arrays, enqueued on `stream` (rtw_tonemap_device)
inline void tonemap_device(const float* d_rgb_sum, uint32_t n_pixels, uint32_t spp, uint8_t* d_rgb8, int device = -1,
                           void* stream = nullptr) {
  check(rtw_tonemap_device(device, d_rgb_sum, n_pixels, spp, d_rgb8, stream));
}
// The per-tile noise estimate of full-layout device sums holding `samples` samples per pixel, enqueued on `stream`
// (rtw_tile_noise_device): d_err (and d_tile_samples, or nullptr) by global tile id, the ids of the tiles above the
// threshold in input order to d_ids_out, their number to *d_n_out; d_ids_in = nullptr tests tiles 0 .. n_in - 1
inline void tile_noise_device(const float* d_sum, const float* d_sq, uint32_t w, uint32_t h, const uint32_t* d_ids_in,
                              uint32_t n_in, uint32_t samples, float threshold, float* d_err, uint32_t* d_tile_samples,
                              uint32_t* d_ids_out, uint32_t* d_n_out, int device = -1, void* stream = nullptr) {
  check(rtw_tile_noise_device(device, d_sum, d_sq, w, h, d_ids_in, n_in, samples, threshold, d_err, d_tile_samples,
                              d_ids_out, d_n_out, stream));
}
// rtw_tonemap with a sample count per 8x8 tile (rtw_tonemap_tiles), and over device arrays (rtw_tonemap_tiles_device)
inline std::vector<uint8_t> tonemap_tiles(const std::vector<float>& sums, uint32_t w, uint32_t h,
                                          const std::vector<uint32_t>& tile_samples) {
  std::vector<uint8_t> out((size_t)w * h * 3);
  check(rtw_tonemap_tiles(sums.data(), w, h, tile_samples.data(), out.data()));
  return out;
}
inline void tonemap_tiles_device(const float* d_rgb_sum, uint32_t w, uint32_t h, const uint32_t* d_tile_samples,
                                 uint8_t* d_rgb8, int device = -1, void* stream = nullptr) {
  check(rtw_tonemap_tiles_device(device, d_rgb_sum, w, h, d_tile_samples, d_rgb8, stream));
}

// The denoiser (include/rtw.h defines the filter): its starting point, as the Python layer's and rtw_console's
constexpr uint32_t DENOISE_ITERATIONS = 5;
constexpr float DENOISE_SIGMA_L = 4.0f, DENOISE_SIGMA_N = 0.5f, DENOISE_SIGMA_Z = 0.1f;
// the device scratch denoise_device needs for a w x h image (rtw_denoise_scratch_bytes; host only)
inline uint64_t denoise_scratch_bytes(uint32_t w, uint32_t h) {
  uint64_t bytes = 0;
  check(rtw_denoise_scratch_bytes(w, h, &bytes));
  return bytes;
}
// The edge-avoiding a-trous filter over full-layout device sums holding `samples` samples per pixel (or
// d_tile_samples[tile]), enqueued on `stream` (rtw_denoise_device): colour sums and, each or nullptr, the sums of
// squares and render_features_device's albedo, normal and depth -> mean radiance, 3 floats per pixel, at d_out
inline void denoise_device(const float* d_sum, const float* d_sq, const float* d_albedo, const float* d_normal,
                           const float* d_depth, uint32_t w, uint32_t h, uint32_t samples, float* d_out,
                           void* d_scratch, const uint32_t* d_tile_samples = nullptr,
                           uint32_t iterations = DENOISE_ITERATIONS, float sigma_l = DENOISE_SIGMA_L,
                           float sigma_n = DENOISE_SIGMA_N, float sigma_z = DENOISE_SIGMA_Z, int device = -1,
                           void* stream = nullptr) {
  check(rtw_denoise_device(device, d_sum, d_sq, d_albedo, d_normal, d_depth, w, h, samples, d_tile_samples, iterations,
                           sigma_l, sigma_n, sigma_z, d_out, d_scratch, stream));
}
// the same arithmetic over host arrays, no GPU (rtw_denoise) -> mean radiance, w * h * 3 floats
inline std::vector<float> denoise(const float* sum, const float* sq, const float* albedo, const float* normal,
                                  const float* depth, uint32_t w, uint32_t h, uint32_t samples,
                                  const uint32_t* tile_samples = nullptr, uint32_t iterations = DENOISE_ITERATIONS,
                                  float sigma_l = DENOISE_SIGMA_L, float sigma_n = DENOISE_SIGMA_N,
                                  float sigma_z = DENOISE_SIGMA_Z) {
  std::vector<float> out((size_t)w * h * 3);
  check(rtw_denoise(sum, sq, albedo, normal, depth, w, h, samples, tile_samples, iterations, sigma_l, sigma_n, sigma_z,
                    out.data()));
  return out;
}

// Temporal accumulation (include/rtw.h defines the operation): its starting point, as the Python layer's and
// rtw_console's, not a tuned result.  max_history = TEMPORAL_MAX_HISTORY_FRAMES * spp.
constexpr uint32_t TEMPORAL_MAX_HISTORY_FRAMES = 32;
constexpr float TEMPORAL_TOL_Z = 0.05f, TEMPORAL_COS_N = 0.9f;
// An accumulated frame's buffers, device or host alike: sum, sq, albedo, normal (3 floats per pixel), depth (2) and
// count (1: the effective samples the other five hold; not read in a current frame).  sq, albedo and normal may be
// nullptr.  FrameOut: the same to write.
struct FrameView {
  const float *sum, *sq, *albedo, *normal, *depth, *count;
};
struct FrameOut {
  float *sum, *sq, *albedo, *normal, *depth, *count;
};
// rtw_temporal's result on the host (a triple out of use stays empty)
struct AccumulatedFrame {
  std::vector<float> sum, sq, albedo, normal, depth, count;
  FrameView view() const {
    auto p = [](const std::vector<float>& v) { return v.empty() ? nullptr : v.data(); };
    return FrameView{p(sum), p(sq), p(albedo), p(normal), p(depth), p(count)};
  }
};
// The current frame (`samples` per pixel, or d_tile_samples[tile]; rendered with cam), plus the history reprojected
// from hist_cam onto cam with at most max_history effective samples -> out, enqueued on `stream`
// (rtw_temporal_device).  hist = nullptr: no history.  An out buffer may be its current-frame buffer, never a history
// buffer.
inline void temporal_device(const FrameView& cur, uint32_t w, uint32_t h, uint32_t samples, const Camera& cam,
                            const FrameView* hist, const Camera* hist_cam, const FrameOut& out, float max_history,
                            float tol_z = TEMPORAL_TOL_Z, float cos_n = TEMPORAL_COS_N,
                            const uint32_t* d_tile_samples = nullptr, int device = -1, void* stream = nullptr) {
  const FrameView none{};
  const FrameView& hv = hist ? *hist : none;
  check(rtw_temporal_device(device, cur.sum, cur.sq, cur.albedo, cur.normal, cur.depth, w, h, samples, d_tile_samples,
                            &cam.c, hv.sum, hv.sq, hv.albedo, hv.normal, hv.depth, hv.count,
                            hist_cam ? &hist_cam->c : nullptr, max_history, tol_z, cos_n, out.sum, out.sq, out.albedo,
                            out.normal, out.depth, out.count, stream));
}
// the same arithmetic over host arrays, no GPU (rtw_temporal) -> the accumulated frame
inline AccumulatedFrame temporal(const FrameView& cur, uint32_t w, uint32_t h, uint32_t samples, const Camera& cam,
                                 const FrameView* hist, const Camera* hist_cam, float max_history,
                                 float tol_z = TEMPORAL_TOL_Z, float cos_n = TEMPORAL_COS_N,
                                 const uint32_t* tile_samples = nullptr) {
  const size_t px = (size_t)w * h;
  AccumulatedFrame f;
  f.sum.resize(px * 3), f.depth.resize(px * 2), f.count.resize(px);
  if (cur.sq) f.sq.resize(px * 3);
  if (cur.albedo) f.albedo.resize(px * 3);
  if (cur.normal) f.normal.resize(px * 3);
  auto p = [](std::vector<float>& v) { return v.empty() ? nullptr : v.data(); };
  const FrameView none{};
  const FrameView& hv = hist ? *hist : none;
  check(rtw_temporal(cur.sum, cur.sq, cur.albedo, cur.normal, cur.depth, w, h, samples, tile_samples, &cam.c, hv.sum,
                     hv.sq, hv.albedo, hv.normal, hv.depth, hv.count, hist_cam ? &hist_cam->c : nullptr, max_history,
                     tol_z, cos_n, p(f.sum), p(f.sq), p(f.albedo), p(f.normal), p(f.depth), p(f.count)));
  return f;
}
// The denoiser for an accumulated frame: its count per pixel in place of `samples` (rtw_denoise_counts_device; scratch
// as denoise_device's)
inline void denoise_counts_device(const FrameView& f, uint32_t w, uint32_t h, float* d_out, void* d_scratch,
                                  uint32_t iterations = DENOISE_ITERATIONS, float sigma_l = DENOISE_SIGMA_L,
                                  float sigma_n = DENOISE_SIGMA_N, float sigma_z = DENOISE_SIGMA_Z, int device = -1,
                                  void* stream = nullptr) {
  check(rtw_denoise_counts_device(device, f.sum, f.sq, f.albedo, f.normal, f.depth, f.count, w, h, iterations, sigma_l,
                                  sigma_n, sigma_z, d_out, d_scratch, stream));
}
// the same arithmetic over host arrays, no GPU (rtw_denoise_counts) -> mean radiance, w * h * 3 floats
inline std::vector<float> denoise_counts(const FrameView& f, uint32_t w, uint32_t h,
                                         uint32_t iterations = DENOISE_ITERATIONS, float sigma_l = DENOISE_SIGMA_L,
                                         float sigma_n = DENOISE_SIGMA_N, float sigma_z = DENOISE_SIGMA_Z) {
  std::vector<float> out((size_t)w * h * 3);
  check(rtw_denoise_counts(f.sum, f.sq, f.albedo, f.normal, f.depth, f.count, w, h, iterations, sigma_l, sigma_n,
                           sigma_z, out.data()));
  return out;
}

}  // namespace rtw
