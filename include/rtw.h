/*
 * rtw.h — C-ABI of the MI355X-native render core (librtw_amd.so).
 *
 * Drop-in boundary for raytracer_weekend_lib's render hot path
 * (reference: /root/reference, paths below relative to raytracer_weekend_lib/src/).
 * The reference boundary is
 *     Raytracer::new(world: &[Box<dyn Hittable>], cam: &Camera, background: Color,
 *                    image_width: u32, image_height: u32, samples_per_pixel: u32)   lib.rs:40-48
 *     Raytracer::render(&self) -> impl RenderIterator<Item = Pixel>                  lib.rs:57-76
 * with the scene built through the Hittable/Material/Texture constructors listed per
 * function below.  Because `dyn Hittable` has no introspection, the world crosses this
 * boundary as a builder call stream (one call per reference constructor), is flattened
 * once by rtw_scene_commit(), and rendered by rtw_render*().  INTEGRATION.md shows the
 * Rust `extern "C"` block and the per-type `flatten` method a maintainer would add.
 *
 * Conventions: every int-returning function returns 0 on success or a negative
 * errno-style code (RTW_E*), with a thread-local message in rtw_last_error().  The
 * reference panics in the same situations (bvh.rs:57, material.rs:71, triangular.rs:178).
 * Input arrays are copied; the caller keeps ownership.  A scene is immutable after
 * rtw_scene_commit(); rendering is blocking on the given (or default) HIP stream.
 * There is no CPU fallback: without a usable gfx950 device rtw_scene_commit() and the
 * render calls fail with RTW_ENODEV.
 */
#ifndef RTW_H
#define RTW_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_ABI_VERSION 7

enum {
  RTW_OK = 0,
  RTW_EINVAL = -22,  /* bad argument (reference: panic / assert) */
  RTW_ENOMEM = -12,
  RTW_ENODEV = -19,  /* no HIP device / kernel launch failed */
  RTW_ESTATE = -71,  /* call not valid in the scene's state (e.g. add after commit) */
  RTW_EIO = -5       /* file / parse error (reference: unwrap on io / parse errors) */
};

typedef struct rtw_scene rtw_scene;

/* camera.rs:9-20 Camera — filled by rtw_camera_new (camera.rs:25-64). */
typedef struct {
  float origin[3], lower_left_corner[3], horizontal[3], vertical[3];
  float u[3], v[3], w[3];
  float lens_radius, time0, time1;
} rtw_camera;

/* Render statistics. rays = number of world.hit queries (lib.rs:102). */
typedef struct {
  uint64_t rays;
  uint64_t paths;          /* W*H*spp actually rendered */
  double kernel_ms;        /* device time of the render kernel(s), HIP events */
  double total_ms;         /* host wall time of the call (incl. D2H for rtw_render) */
  uint64_t node_visits;    /* only when RTW_FLAG_COUNT_TRAVERSAL */
  uint64_t prim_tests;     /* only when RTW_FLAG_COUNT_TRAVERSAL */
  uint64_t prim_tests_by_type[6]; /* sphere, moving sphere, rect xy, xz, yz, triangle */
  /* RTW_FLAG_COUNT_TRAVERSAL: SIMD utilisation, pairs of (wave executions, active lanes) for
   * the BVH node loop, primitive tests and path segments */
  uint64_t simd[6];
  /* RTW_FLAG_COUNT_TRAVERSAL: wave-cycles (s_memtime) spent in path regeneration, closest-hit
   * traversal and shading, and in the whole path kernel, summed over waves */
  uint64_t phase_cycles[4];
  /* RTW_FLAG_COUNT_TRAVERSAL: child boxes slab-tested (the non-empty slots of the visited 4-wide
   * nodes), and sub-phase wave-cycles: [0] shading's random_in_unit_sphere (counted apart from
   * phase_cycles[2]), [1] traversal's node loop and [2] leaf tests (parts of phase_cycles[1]),
   * [3] regeneration's per-lane path start (part of phase_cycles[0]) */
  uint64_t boxes_tested;
  uint64_t sub_cycles[4];
} rtw_stats;

enum {
  RTW_FLAG_COUNT_TRAVERSAL = 1,
  /* rtw_render_samples_device with d_tile_ids: d_sum and d_sq are full w x h x 3 images, each named tile at its place */
  RTW_FLAG_FULL_IMAGE = 2
};

const char* rtw_last_error(void);
int rtw_abi_version(void);
/* Number of visible HIP devices (0 in a GPU-less container; never initialises a context). */
int rtw_device_count(void);

/* ---- scene lifetime */
int rtw_scene_create(rtw_scene** out);
void rtw_scene_destroy(rtw_scene* scene);

/* ---- textures: texture.rs:45-60 SolidColor::new/new_rgb, :62-81 Checker::new(odd, even, freq),
 *      image_texture.rs:23-30 ImageTexture (decoded RGB8 pixels, row-major, top row first),
 *      texture.rs:97-104 UVDebug */
int rtw_texture_solid(rtw_scene* s, float r, float g, float b, uint32_t* id);
int rtw_texture_checker(rtw_scene* s, uint32_t odd, uint32_t even, float frequency, uint32_t* id);
int rtw_texture_image(rtw_scene* s, const uint8_t* rgb8, uint32_t width, uint32_t height, uint32_t* id);
int rtw_texture_uvdebug(rtw_scene* s, uint32_t* id);
/* texture.rs:83-95 Noise::new(Perlin, scale): value = 0.5 (1 + sin(scale p.z + 10 turbulence(p, 7))).
 * The Perlin tables (perlin.rs:8-48) cross as data: gradients 256x3 floats (unit vectors),
 * permutations 3x256 (x, y, z; each a permutation of 0..255, else RTW_EINVAL).  Perlin::new(rng)
 * with this build's seeded stream is rtw_perlin_generate(). */
int rtw_texture_noise(rtw_scene* s, const float* gradients, const uint32_t* permutations, float scale,
                      uint32_t* id);
int rtw_perlin_generate(uint64_t seed, float* gradients, uint32_t* permutations);

/* ---- materials: material.rs:30-39 Lambertian::new, :63-73 Metal::new (fuzz <= 1 else
 *      RTW_EINVAL, as the assert at :71), :102-105 Dielectric::new, light_source.rs:12-15
 *      DiffuseLight::new */
int rtw_material_lambertian(rtw_scene* s, uint32_t texture, uint32_t* id);
int rtw_material_metal(rtw_scene* s, float r, float g, float b, float fuzz, uint32_t* id);
int rtw_material_dielectric(rtw_scene* s, float index_of_refraction, uint32_t* id);
int rtw_material_diffuse_light(rtw_scene* s, uint32_t texture, uint32_t* id);
/* material.rs:148-165 Isotropic::new(albedo texture): scatters into random_in_unit_sphere */
int rtw_material_isotropic(rtw_scene* s, uint32_t texture, uint32_t* id);

/* ---- hierarchy.  Objects are appended to the innermost open group (the world list at the
 *      top).  Groups nest; each must be closed with rtw_end().
 *      rtw_begin_list:      Vec<Box<dyn Hittable>>            hittable/mod.rs:57-69, 90-98
 *      rtw_begin_bvh:       BvhNode::new(objects, t0, t1, rng)  bvh.rs:19-74
 *      rtw_begin_translate: Translation::new(inner, offset)    transformations.rs:16-47
 *      rtw_begin_rotate_y:  YRotation::new(inner, degrees)     transformations.rs:50-75
 *      rtw_begin_constant_medium: ConstantMedium::new(boundary, density, texture) volumes.rs:17-35;
 *        the group holds the boundary: exactly one object, a Sphere or a Cuboid (optionally under
 *        Translation / YRotation) in this build, else RTW_EINVAL at rtw_end / commit.  Creates the
 *        medium's Isotropic(texture) phase function, whose id goes to *material (may be NULL).
 *        The medium's free-path draw comes from a sub-stream keyed by (path segment, medium),
 *        not the path's shared stream (order-independent form).
 *      A wrapper applies to everything added inside it (= the wrapper of a list). */
int rtw_begin_list(rtw_scene* s);
int rtw_begin_bvh(rtw_scene* s, float time0, float time1);
int rtw_begin_translate(rtw_scene* s, float x, float y, float z);
int rtw_begin_rotate_y(rtw_scene* s, float degrees);
int rtw_begin_constant_medium(rtw_scene* s, float density, uint32_t texture, uint32_t* material);
int rtw_end(rtw_scene* s);

/* ---- primitives (SoA arrays of length n; copied)
 *      Sphere::new(center, radius, material)                spherical.rs:79-104
 *      MovingSphere::new(c0, t0, c1, t1, radius, material)  spherical.rs:106-151
 *      XY/XZ/YZRectangle::new(a0, a1, b0, b1, k, material)  rectangular.rs:16-166
 *        axis: 0 = XY (k on z), 1 = XZ (k on y), 2 = YZ (k on x)
 *      Cuboid::new(p0, p1, material)                        rectangular.rs:170-245
 *      Triangle::new(vertices, [Option<normal>;3], [Option<uv>;3], material)  triangular.rs:33-73
 *        verts: 9n floats; normals: 9n floats or NULL; normal_mask: n bytes (bit k = vertex k
 *        has a normal) or NULL; uvs: 6n floats or NULL; uv_mask likewise. */
int rtw_add_spheres(rtw_scene* s, uint32_t n, const float* cx, const float* cy, const float* cz,
                    const float* radius, const uint32_t* material);
int rtw_add_moving_spheres(rtw_scene* s, uint32_t n, const float* c0x, const float* c0y,
                           const float* c0z, const float* t0, const float* c1x, const float* c1y,
                           const float* c1z, const float* t1, const float* radius,
                           const uint32_t* material);
int rtw_add_rects(rtw_scene* s, uint32_t n, const uint32_t* axis, const float* a0, const float* a1,
                  const float* b0, const float* b1, const float* k, const uint32_t* material);
int rtw_add_cuboid(rtw_scene* s, const float p0[3], const float p1[3], uint32_t material);
int rtw_add_triangles(rtw_scene* s, uint32_t n, const float* verts, const float* normals,
                      const uint8_t* normal_mask, const float* uvs, const uint8_t* uv_mask,
                      uint32_t material);

/* load_wavefront_obj(path, rng) triangular.rs:241-260: adds BvhNode(triangles) to the open
 * group.  Faces without a material get DiffuseLight(1,0,1) (:177-182); map_Kd images are
 * decoded only if image_loader != NULL (the build ships no JPEG/PNG decoder; a missing
 * loader or file is RTW_EIO as the reference's unwrap at :308).  `.rtwm` files (this
 * build's binary mesh dump) are accepted too; their material is taken
 * from `fallback_material` when != UINT32_MAX. */
typedef int (*rtw_image_loader)(const char* path, uint8_t** rgb8, uint32_t* w, uint32_t* h);
int rtw_load_wavefront_obj(rtw_scene* s, const char* path, rtw_image_loader image_loader,
                           uint32_t fallback_material, uint32_t* n_triangles);

/* Flatten the hierarchy, build the BVH and upload to every visible device (or only to
 * `device` when >= 0).  After this the scene is immutable. */
int rtw_scene_commit(rtw_scene* s, int device);

/* Camera::new(look_from, look_at, vup, vfov, aspect, aperture, focus_dist, t0, t1) camera.rs:25-64 */
int rtw_camera_new(const float look_from[3], const float look_at[3], const float vup[3],
                   float vfov_degrees, float aspect_ratio, float aperture, float focus_dist,
                   float time0, float time1, rtw_camera* out);

/* Raytracer::new(world, cam, background, w, h, spp).render().collect() — lib.rs:40-95.
 * out_rgb_sum (host, w*h*3 floats) receives the un-normalised Σ over spp per pixel in the
 * reference's emission order (lib.rs:58: row j = h-1 .. 0, column i = 0 .. w-1), i.e.
 * out[((h-1-j)*w + i)*3 + c].  max_depth is MAX_DEPTH (lib.rs:32, 50).  The per-sample
 * random stream is keyed by (seed, j, i, sample) so the image is independent of tiling
 * and device count. */
int rtw_render(rtw_scene* s, const rtw_camera* cam, const float background[3], uint32_t w,
               uint32_t h, uint32_t spp, uint32_t max_depth, uint64_t seed, float* out_rgb_sum,
               rtw_stats* stats);

/* lib.rs:120-126 Pixel: row j (0 = bottom), column i, un-normalised Σ over spp. */
typedef struct {
  uint32_t row, column;
  float color[3];
} rtw_pixel;
/* Receives the next n pixels of the stream; a non-zero return stops the render (returned as is). */
typedef int (*rtw_pixel_sink)(const rtw_pixel* pixels, uint32_t n, void* user);

/* Raytracer::render() as a progressive stream (lib.rs:50-76 RenderIterator): the frame is rendered
 * in bands of `band_rows` output rows (rounded up to whole 8-row tile rows; 0 = 64) and each band's
 * pixels are handed to `sink` in the reference's emission order (row j = h-1 .. 0, column 0 .. w-1)
 * as soon as the band is done.  Same pixels as rtw_render. */
int rtw_render_stream(rtw_scene* s, const rtw_camera* cam, const float background[3], uint32_t w,
                      uint32_t h, uint32_t spp, uint32_t max_depth, uint64_t seed, uint32_t band_rows,
                      rtw_pixel_sink sink, void* user, rtw_stats* stats);

/* lib.rs:128-138 ProgressMessage on the wire (discovery_app/src/bin/raytracer.rs:62-113 ->
 * discovery_host_receiver/src/main.rs:22-110): postcard 0.7.3 (Cargo.lock:2533-2541; enum tag and
 * u32 as varints, f32 little-endian, Color as its 3-float array) framed by COBS (postcard-cobs
 * 0.1.5-pre) with a trailing 0x00, exactly as postcard::to_vec_cobs. */
enum { RTW_MSG_IMAGE_START = 0, RTW_MSG_PIXEL = 1, RTW_MSG_IMAGE_END = 2 };
typedef struct {
  uint32_t kind;
  uint32_t width, height, samples_per_pixel; /* RTW_MSG_IMAGE_START */
  rtw_pixel pixel;                           /* RTW_MSG_PIXEL */
} rtw_progress_msg;
/* Encodes one message (<= 32 bytes incl. the 0x00 delimiter) into out; *len = bytes written. */
int rtw_progress_encode(const rtw_progress_msg* msg, uint8_t* out, size_t cap, size_t* len);
/* Decodes one COBS frame (with or without its trailing 0x00), as postcard::from_bytes_cobs. */
int rtw_progress_decode(const uint8_t* frame, size_t len, rtw_progress_msg* msg);

/* Render a subset of 8x8 pixel tiles into device memory (multi-GPU / framework path).
 * Tile t covers columns [8*tx, 8*tx+8) and output rows [8*ty, 8*ty+8) (row r <-> j = h-1-r),
 * tile id = ty * ceil(w/8) + tx.  If d_tile_ids == NULL all tiles are rendered and d_out is a
 * full w*h*3 image in reference order; otherwise d_tile_ids is a DEVICE array of n_tiles ids
 * and d_out is packed [n_tiles][64][3] (pixels outside the image, and ids beyond the last tile,
 * are left untouched).  `stream` is a hipStream_t (NULL = default).  The call only enqueues unless
 * stats != NULL, in which case it synchronises and fills stats.  Each (scene, device) pair owns one
 * path queue and one sample buffer: renders of a scene on one device must be serialised on one
 * stream (two renders in flight on different streams would share them); so must its ray queries
 * (rtw_hit_rays*), which share the traversal-stack spill area with them.  The first render of a
 * given size allocates the sample buffer (hipMalloc: not stream-capturable); later renders of the
 * same or a smaller size only enqueue.  Without stats, a traversal fault of this render surfaces at
 * the first rtw_render* call that starts after this render has COMPLETED (the check reads the device's
 * host-mapped error word without waiting), or at rtw_render_status, which waits. */
int rtw_render_device(rtw_scene* s, int device, const rtw_camera* cam, const float background[3],
                      uint32_t w, uint32_t h, uint32_t spp, uint32_t max_depth, uint64_t seed,
                      const uint32_t* d_tile_ids, uint32_t n_tiles, float* d_out, void* stream,
                      uint32_t flags, rtw_stats* stats);
/* rtw_render_device over the tiles first_tile + k * tile_stride (k < n_tiles) without an id table
 * (the kernel computes them): a device's round-robin share of the frame (rtw_tile_partition part p of
 * n: first_tile = p, tile_stride = n).  d_out is packed [n_tiles][64][3].  RTW_EINVAL if a tile
 * leaves the frame or tile_stride == 0. */
int rtw_render_device_strided(rtw_scene* s, int device, const rtw_camera* cam, const float background[3],
                              uint32_t w, uint32_t h, uint32_t spp, uint32_t max_depth, uint64_t seed,
                              uint32_t first_tile, uint32_t tile_stride, uint32_t n_tiles, float* d_out,
                              void* stream, uint32_t flags, rtw_stats* stats);

/* ---- progressive renders: more samples onto a frame that exists (preview at 1, 2, 4 ... spp, resuming, spreading a
 *      frame over time), with the per-pixel sum of squares for a noise estimate.  The path generator is keyed by
 *      (seed, j, i, sample) and a frame is the in-order f32 sum over its samples, so samples [a, b) added onto the sums
 *      of [0, a) are rtw_render's frame of b samples bit for bit, with the same number of rays, however [0, b) is cut. */
/* Samples [sample_first, sample_first + n_samples) of every pixel of the tile set, ADDED in sample order onto what
 * d_sum (and d_sq, may be NULL) hold: zeroed buffers = a fresh frame.  d_sq, a second device buffer of d_sum's layout,
 * receives per channel m = m + (x * x) in the same order (two f32 roundings).  Tile arguments, layouts, stream, flags
 * and stats as rtw_render_device; pixels outside the image, tiles not named and ids beyond the last tile are left
 * untouched in both buffers.  Checks in the render calls' order: a NULL argument (RTW_EINVAL), an uncommitted scene
 * (RTW_ESTATE), an image under 2x2, then sample_first + n_samples > 2^31 (both RTW_EINVAL), then the device copy
 * (RTW_ENODEV).  n_samples = 0 or max_depth = 0 is RTW_OK and leaves both buffers untouched (every such sample is
 * black, and adding +0 would only turn a -0 into +0).  The range runs as the aligned power-of-two blocks of
 * rtw_sample_blocks, each an ordinary pass of the scene's path kernel: stats->rays sums them.  The call shares the
 * (scene, device) pair's path queue, sample buffer (grown for the largest block) and spill area: it must be serialised
 * with the pair's renders and queries on one stream, as rtw_render_device. */
int rtw_render_samples_device(rtw_scene* s, int device, const rtw_camera* cam, const float background[3],
                              uint32_t w, uint32_t h, uint32_t sample_first, uint32_t n_samples,
                              uint32_t max_depth, uint64_t seed, const uint32_t* d_tile_ids, uint32_t n_tiles,
                              float* d_sum, float* d_sq, void* stream, uint32_t flags, rtw_stats* stats);
/* host only: the aligned power-of-two blocks the call above runs, in order (block k = [first[k], first[k] + 2^log2[k]),
 * first[k] a multiple of its size): at each position the largest such block that fits what is left, hence at most 62.
 * *n_blocks = their number; RTW_EINVAL if cap is smaller (nothing written) or the range goes beyond 2^31. */
int rtw_sample_blocks(uint32_t sample_first, uint32_t n_samples, uint32_t* first, uint32_t* log2, uint32_t cap,
                      uint32_t* n_blocks);
/* Receives the frame after a step: host copies (they belong to the call) of the sums and sums of squares in
 * rtw_render's layout, and the samples per pixel they hold.  A non-zero return stops the render (returned as is). */
typedef int (*rtw_frame_sink)(const float* rgb_sum, const float* rgb_sq_sum, uint32_t w, uint32_t h,
                              uint32_t samples_done, void* user);
/* Blocking, first device copy: a frame of spp samples (<= 2^31) in growing steps, the sink called after each with host
 * copies of both sums; a non-zero return stops the render and is returned as is.  step = 0: the steps end at 1, 2, 4,
 * 8, ... samples and then at spp; step > 0: doubling while the doubled count is within step, then step samples at a
 * time (a power-of-two step keeps every chunk but the last one block of rtw_sample_blocks).  The last call's rgb_sum
 * is rtw_render's image.  The device sums live in buffers the device copy keeps (grown once).  stats: totals over the
 * whole call.  spp = 0 calls the sink never.  Checks as above, `sink` among the NULL arguments.  (`sink` is an
 * rtw_frame_sink, its type written out: the header parser of tests/test_integration_abi.py lists the prototypes whose
 * parameter types it knows by name, and tests/test_render_samples_abi.py holds this one against the typedef.) */
int rtw_render_progressive(rtw_scene* s, const rtw_camera* cam, const float background[3], uint32_t w, uint32_t h,
                           uint32_t spp, uint32_t max_depth, uint64_t seed, uint32_t step,
                           int (*sink)(const float* rgb_sum, const float* rgb_sq_sum, uint32_t w, uint32_t h,
                                       uint32_t samples_done, void* user),
                           void* user, rtw_stats* stats);
/* rtw_tonemap (below) from a DEVICE sum image to a DEVICE RGB8 image on `stream`, byte for byte: a preview then costs
 * 3 B per pixel to copy.  Only enqueues.  device < 0: the current device.  RTW_EINVAL: a NULL buffer with n_pixels > 0,
 * spp = 0. */
int rtw_tonemap_device(int device, const float* d_rgb_sum, uint32_t n_pixels, uint32_t spp, uint8_t* d_rgb8,
                       void* stream);

/* ---- adaptive sampling: the sample count follows a per-tile noise estimate made from the two sums above.  A tile
 *      that stopped at n samples holds exactly rtw_render's pixels of an n-spp frame (same seed), since samples are
 *      only ever added in order: every parity guarantee of the fixed-spp frame carries over tile by tile.
 *      The estimate of an 8x8 tile whose pixels hold n samples, all in f32, one rounding per operation, inv = 1.0f / n:
 *      per in-image pixel and channel c  m_c = s_c inv,  v_c = max0(q_c inv - m_c m_c)  (a NaN stays a NaN);
 *      e = (v_0 + v_1) + v_2, l = (m_0 + m_1) + m_2, and +0 for the pixels of a ragged tile that are off the image;
 *      E, L = the sums of the tile's 64 e and l (pixel (x, y) of the tile at index 8 y + x) by the adjacent-pair tree
 *      (level k = 0..5: x[i] = x[i] + x[i ^ (1 << k)]);  Pf = the tile's in-image pixels;
 *      err = sqrt((E inv) / Pf) / (|L| / Pf + 0.03).   The tile is converged iff err <= threshold (a NaN never is). */
/* The estimate of n_in tiles of the DEVICE images d_sum / d_sq (full w x h x 3 layout, `samples` >= 1 samples in every
 * tested pixel), on `stream`; only enqueues.  d_ids_in: device tile ids, NULL = the tiles 0 .. n_in - 1 (n_in = the
 * tile count: every tile); an id beyond the last tile is skipped.  d_err[tile] = err and, unless NULL,
 * d_tile_samples[tile] = samples, both by global tile id and for tested tiles only.  d_ids_out receives the ids of the
 * tiles NOT converged, in input order (an ascending list stays ascending), *d_n_out their number; d_ids_out needs room
 * for n_in ids, serves as the call's scratch and must not overlap d_ids_in.  device < 0: the current device.
 * RTW_EINVAL: a NULL buffer (d_ids_in and d_tile_samples excepted), an image under 2x2 or over 65536 a side,
 * samples == 0, a threshold that is NaN, negative or infinite. */
int rtw_tile_noise_device(int device, const float* d_sum, const float* d_sq, uint32_t w, uint32_t h,
                          const uint32_t* d_ids_in, uint32_t n_in, uint32_t samples, float threshold, float* d_err,
                          uint32_t* d_tile_samples, uint32_t* d_ids_out, uint32_t* d_n_out, void* stream);
/* A fresh frame (d_sum and d_sq, full w x h x 3 device images, are zeroed first) whose tiles stop when converged.
 * Rounds end at n_0 = min_spp, n_{k+1} = min(2 n_k, max_spp) samples per pixel: each adds the missing samples to the
 * tiles still active (rtw_render_samples_device with their ids and RTW_FLAG_FULL_IMAGE), then tests them as above; the
 * tiles not converged go on, until max_spp.  d_tile_samples[tiles]: the samples each tile holds; d_tile_err[tiles] (may
 * be NULL): its last estimate.  Blocking on `stream`: one 4-byte count is read back per round.  Checks in the render
 * calls' order: a NULL argument (d_sq and d_tile_samples included), the scene's state, an image under 2x2, then
 * 2 <= min_spp <= max_spp <= 2^31 and the threshold as above (RTW_EINVAL), then the device copy (RTW_ENODEV).
 * max_depth = 0 leaves zeros, every tile converged at min_spp.  flags: RTW_FLAG_COUNT_TRAVERSAL.  stats: rays and
 * kernel_ms summed over the rounds (the tests' kernels included), paths = 64 x the sum of d_tile_samples.  Serialised
 * with the (scene, device) pair's other renders, as rtw_render_samples_device. */
int rtw_render_adaptive_device(rtw_scene* s, int device, const rtw_camera* cam, const float background[3],
                               uint32_t w, uint32_t h, uint32_t min_spp, uint32_t max_spp, uint32_t max_depth,
                               uint64_t seed, float threshold, float* d_sum, float* d_sq, uint32_t* d_tile_samples,
                               float* d_tile_err, void* stream, uint32_t flags, rtw_stats* stats);
/* The host form, on the first device copy: rgb_sum[w*h*3], rgb_sq_sum[w*h*3] (may be NULL), tile_samples[tiles],
 * tile_err[tiles] (may be NULL) are host arrays.  The device images live in buffers the device copy keeps. */
int rtw_render_adaptive(rtw_scene* s, const rtw_camera* cam, const float background[3], uint32_t w, uint32_t h,
                        uint32_t min_spp, uint32_t max_spp, uint32_t max_depth, uint64_t seed, float threshold,
                        float* rgb_sum, float* rgb_sq_sum, uint32_t* tile_samples, float* tile_err, rtw_stats* stats);
/* rtw_tonemap_tiles (below) from DEVICE arrays to a DEVICE RGB8 image on `stream`, byte for byte; only enqueues.
 * device < 0: the current device.  RTW_EINVAL: a NULL buffer, an image under 2x2 or over 65536 a side. */
int rtw_tonemap_tiles_device(int device, const float* d_rgb_sum, uint32_t w, uint32_t h,
                             const uint32_t* d_tile_samples, uint8_t* d_rgb8, void* stream);

/* ---- feature buffers: what a denoiser behind a few-sample frame wants as guides -- first-hit albedo, normal and
 *      depth per pixel, summed over the pixel's camera rays.  For pixel (j, i) and sample s the ray is rtw_camera_rays'
 *      ray for (seed, j, i, s) (it does not depend on spp), its stream word the generator's state after the time draw,
 *      and the record what rtw_hit_rays returns for that ray (same walk, same winner; the stream word keys a
 *      ConstantMedium's free path).  The sample's features:
 *        albedo (3 f32): a hit: what rtw_scatter_rays gives as the attenuation of a scattered ray or the emission of a
 *                        light -- a Lambertian's / Isotropic's / DiffuseLight's texture value at (u, v, p), (1, 1, 1)
 *                        for a Dielectric -- and for a Metal its albedo colour whether or not this ray would be
 *                        absorbed (rtw_scatter_rays reports attenuation 0 there); a miss: `background`;
 *        normal (3 f32): rtw_hit::normal as it stands (it faces the ray; not normalised where a triangle interpolates
 *                        vertex normals); a miss: +0;
 *        depth  (2 f32): (t, 1.0f); a miss: (+0, +0).  The second channel sums to the pixel's hit count, its coverage:
 *                        divide by the samples for means, or by the count for the mean depth of what was hit.
 *      No draw is made beyond the camera's.  Each buffer holds, per pixel and channel, x = x + f_s for s in sample order
 *      (one f32 rounding per sample), added onto what it already holds: zeroed buffers give a fresh frame, and samples
 *      [a, b) added onto the sums of [0, a) are the sums of [0, b) bit for bit, however the range is cut -- the property
 *      rtw_render_samples_device's colour sums have, so both cut alike. */
/* Samples [sample_first, sample_first + n_samples) of every pixel of the tile set, ADDED onto the DEVICE buffers: one
 * fused kernel in place of rtw_camera_rays_device -> rtw_hit_rays_device -> rtw_scatter_rays_device and a per-pixel sum.
 * Tile arguments, layouts, stream and RTW_FLAG_FULL_IMAGE as rtw_render_samples_device (tile ids must not repeat);
 * d_albedo and d_normal have d_sum's layout (w*h*3, or packed [n_tiles][64][3]), d_depth two floats per pixel (w*h*2,
 * or packed [n_tiles][64][2]).  Each of the three may be NULL, not all.  Pixels outside the image, tiles not named and
 * ids beyond the last tile are left untouched.  Checks in rtw_render_samples_device's order and with its codes: a NULL
 * argument (all three buffers NULL among them), then a flag other than RTW_FLAG_FULL_IMAGE (both RTW_EINVAL), an
 * uncommitted scene (RTW_ESTATE), an image under 2x2, sample_first + n_samples > 2^31 (RTW_EINVAL), the device copy
 * (RTW_ENODEV), then a pending traversal fault, an image side over 65536 and a camera shutter outside the committed
 * motion range (RTW_EINVAL).  n_samples = 0 is RTW_OK and touches nothing.  The call only enqueues unless
 * stats != NULL; stats: rays = paths = the samples traced, counted on the device, kernel_ms, total_ms.  The kernel is
 * the scene's own variant beside its path kernel; it uses the (scene, device) pair's spill area and counter words, so
 * the call must be serialised with the pair's renders and queries on one stream, as they are among themselves. */
int rtw_render_features_device(rtw_scene* s, int device, const rtw_camera* cam, const float background[3],
                               uint32_t w, uint32_t h, uint32_t sample_first, uint32_t n_samples, uint64_t seed,
                               const uint32_t* d_tile_ids, uint32_t n_tiles, float* d_albedo, float* d_normal,
                               float* d_depth, void* stream, uint32_t flags, rtw_stats* stats);
/* The host form: blocking, on the first device copy; a fresh frame of spp samples (<= 2^31) over every tile into the
 * host arrays albedo[w*h*3], normal[w*h*3], depth[w*h*2] in rtw_render's layout (row r <-> j = h-1-r), i.e.
 * rtw_render_features_device of samples [0, spp) onto zeroed buffers.  Any of the three may be NULL, not all.  The
 * device buffers belong to the device copy and are grown once.  spp = 0 gives zeros. */
int rtw_render_features(rtw_scene* s, const rtw_camera* cam, const float background[3], uint32_t w, uint32_t h,
                        uint32_t spp, uint64_t seed, float* albedo, float* normal, float* depth, rtw_stats* stats);

/* ---- ambient occlusion / sky visibility: per pixel, how many of the short rays cast from its first hits over the
 *      hemisphere reach `radius` unoccluded -- a clay preview that converges at 1-4 samples, a contact-shadow guide.
 *      No counterpart in the reference, so the buffer is DEFINED here, on the other calls' answers.  For pixel (j, i) and
 *      sample s of a w x h frame, with ao_rays = K >= 1 and radius = R > 0:
 *        1. The camera ray and its stream word g_0 are rtw_camera_rays' for (seed, j, i, s) (the ray
 *           rtw_render_features* traces); rec is what rtw_hit_rays returns for it.
 *        2. A miss adds (+0, +0) and makes no draw.
 *        3. A hit casts K AO rays, k = 0 .. K-1 in order.  Direction d_k and next word g_{k+1}: what rtw_scatter_rays
 *           gives as the out ray's direction and stream for rec with its material replaced by a Lambertian and the
 *           ray's stream = g_k (rs = random_in_unit_sphere, d = normal + unit(rs), a near-zero d -> normal).  The real
 *           material is not consulted: a light, glass or a medium casts rays the same way.  The AO ray: origin rec.p,
 *           direction d_k (not normalised), time the camera ray's, stream g_{k+1} (it keys media as for any query).
 *           The bound: len = sqrtf((d_x d_x + d_y d_y) + d_z d_z), T = R / len, IEEE f32, one rounding per operation
 *           (len = 0 or R = +inf: T = +inf, plain sky visibility).  occ_k = rtw_occluded_rays' answer for that ray
 *           and T: hit && !(t > T) on rtw_hit_rays' record (inclusive; a NaN t occludes; T < 0.001 is free but for
 *           that case).
 *        4. The buffer holds two floats per pixel, (open, cast), in d_depth's layout.  Per sample, in sample order:
 *           x_0 = x_0 + (float)(K - sum of occ_k), x_1 = x_1 + (float)K; a miss adds +0 to both.  One f32 rounding per
 *           sample, added onto what the buffer holds: zeroed buffers give a fresh frame, and samples [a, b) added onto
 *           the sums of [0, a) are the sums of [0, b) bit for bit however the range is cut, as the colour and feature
 *           sums.  Mean AO = open / cast (cast = 0: nothing was hit); cast / K is the pixel's hit count.
 *      No draw beyond these.  The AO rays' walk is the scene's own any-hit walk, as rtw_occluded_rays runs it. */
/* Samples [sample_first, sample_first + n_samples) of every pixel of the tile set, ADDED onto the DEVICE buffer d_ao
 * (w*h*2, or packed [n_tiles][64][2]): one fused kernel in place of rtw_camera_rays_device -> rtw_hit_rays_device -> a
 * caller's kernel making the AO rays -> rtw_occluded_rays_device and a per-pixel sum.  Tile arguments, layouts, stream,
 * RTW_FLAG_FULL_IMAGE, what is left untouched and the serialisation rule as rtw_render_features_device (it uses the
 * (scene, device) pair's spill area, error word and counter words).  Checks in that call's order and with its codes: a
 * NULL argument, then a flag other than RTW_FLAG_FULL_IMAGE (both RTW_EINVAL), an uncommitted scene (RTW_ESTATE), an
 * image under 2x2, sample_first + n_samples > 2^31, ao_rays outside 1 .. 256, a radius that is NaN or <= 0 (+inf is
 * valid) (RTW_EINVAL), the device copy (RTW_ENODEV), then a pending traversal fault, an image side over 65536 and a
 * camera shutter outside the committed motion range (RTW_EINVAL).  n_samples = 0 that passed the argument checks is
 * RTW_OK and touches nothing, the device copy included.  The call only enqueues unless stats != NULL; stats: paths =
 * the camera samples traced, rays = paths + the AO rays cast (every world.hit query), both counted on the device,
 * kernel_ms, total_ms. */
int rtw_render_ao_device(rtw_scene* s, int device, const rtw_camera* cam, uint32_t w, uint32_t h,
                         uint32_t sample_first, uint32_t n_samples, uint64_t seed, uint32_t ao_rays, float radius,
                         const uint32_t* d_tile_ids, uint32_t n_tiles, float* d_ao, void* stream, uint32_t flags,
                         rtw_stats* stats);
/* The host form: blocking, on the first device copy; samples [0, spp) (spp <= 2^31) of every tile summed onto a zeroed
 * device buffer the device copy keeps and grows once, copied into ao[w*h*2] in rtw_render's layout (row r <-> j = h-1-r).
 * spp = 0 gives zeros. */
int rtw_render_ao(rtw_scene* s, const rtw_camera* cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                  uint32_t ao_rays, float radius, float* ao, rtw_stats* stats);

/* ---- the denoiser: an edge-avoiding a-trous wavelet filter (a dilated 5x5 B3 spline per iteration) for few-sample
 *      frames, over what the calls above leave on the device: the colour sums and sums of squares of
 *      rtw_render_samples_device / rtw_render_adaptive_device and the guides of rtw_render_features_device.  It
 *      filters the albedo-demodulated mean radiance; its edge stops come from normal, depth and luminance, the last
 *      scaled by the per-pixel variance of the mean, which is carried through the iterations.  No counterpart in the
 *      reference, so
 *      the filter is DEFINED here, operation by operation: all arithmetic f32 with one rounding per operation (no fused
 *      multiply-add), IEEE division and sqrt, no transcendentals; max0(v) is v > 0 ? v : 0 (a NaN gives 0).  The device
 *      kernels, rtw_denoise's host loops and the tests' numpy restatement agree bit for bit.
 *      Inputs, full w x h layout, rows as rtw_render: sum (3 floats per pixel), sq (3, may be NULL), albedo (3, may be
 *      NULL), normal (3, may be NULL), depth (2, may be NULL).  A pixel's sample count n is `samples`, or with a table
 *      tile_samples[t] of the pixel's 8x8 tile, t as rtw_tonemap_tiles finds it; the same n holds for all five buffers
 *      (a progressive or adaptive loop hands both render calls the same ranges).
 *      Prepare, per pixel, inv = 1.0f / (float)n, per channel c:
 *        m_c = s_c * inv;  a_c = A_c * inv;  d_c = a_c > 0.001f ? a_c : 0.001f (1.0f without albedo);  x_c = m_c / d_c;
 *        v_c = q_c * inv - m_c * m_c, v_c < 0 ? 0 : v_c (rtw_tile_noise_device's clamp: a NaN stays);
 *        u_c = (v_c * inv) / (d_c * d_c);  var = (u_0 + u_1) + u_2  (+0 without sq);
 *        nn = (N_0 N_0 + N_1 N_1) + N_2 N_2;  g_c = nn > 0 ? N_c / sqrt(nn) : +0  (+0 without normal);
 *        z = T * inv with T the first depth channel (+0 without depth).
 *      A pixel with n = 0 is empty: x_c a quiet NaN, var, g_c, z = +0, its output +0.
 *      Iteration k = 0 .. iterations - 1, step = 1 << k, for pixel p, with the luminance
 *        l(x) = (0.2126f x_0 + 0.7152f x_1) + 0.0722f x_2:
 *        rz = 1.0f / ((sigma_z * (float)step) * fabsf(z_p) + 1e-6f);  rl = 1.0f / (sigma_l * sqrtf(var_p) + 1e-4f);
 *        k_n = 1.0f / (sigma_n * sigma_n), computed once on the host.
 *      Taps q = p + step * (dx, dy), dy = -2..2 outer, dx = -2..2 inner, those off the image skipped; H = {0.375, 0.25,
 *      0.0625}; the tap's weight, built in this order:
 *        w = H[|dx|] * H[|dy|];
 *        w = w * max0(1 - dn2 * k_n), dn2 = (e_0 e_0 + e_1 e_1) + e_2 e_2, e = g_p - g_q   (dropped for sigma_n = 0);
 *        w = w * max0(1 - fabsf(z_p - z_q) * rz)                                          (dropped for sigma_z = 0);
 *        w = w * max0(1 - fabsf(l(x_p) - l(x_q)) * rl)                     (dropped for sigma_l = 0 or without sq).
 *      A tap counts only if w > 0 and l(x_q) == l(x_q); then sw = sw + w, sx_c = sx_c + w * x_q,c and
 *      sv = sv + (w * w) * var_q, in tap order: the order is the contract.  If sw > 0: x'_c = sx_c / sw and
 *      var' = sv / (sw * sw); otherwise the pixel keeps x and var.  The guides do not change between iterations.
 *      Finish: out_c = x_c * d_c, the mean radiance (rtw_tonemap* with spp = 1 makes the preview); +0 for an empty
 *      pixel.
 *      Both calls answer RTW_EINVAL for, in this order: a NULL sum, out or (device call) scratch; an image under 2x2
 *      or over 65536 a side; samples = 0 without a tile table; iterations > 10; a sigma that is NaN, negative or
 *      infinite (sigma_l, sigma_n, sigma_z in turn).  iterations = 0 is valid: prepare, then finish. */
/* The bytes of device scratch rtw_denoise_device needs for a w x h image (host only; the only place that knows the
 * size: the ping-pong images and the prepared guides).  RTW_EINVAL: bytes NULL, then an image under 2x2 or over 65536
 * a side. */
int rtw_denoise_scratch_bytes(uint32_t w, uint32_t h, uint64_t* bytes);
/* The filter over DEVICE arrays, enqueued on `stream` (no scene: what rtw_tonemap_device is to rtw_tonemap).
 * device < 0 means the current device.  d_out (w*h*3 floats) may not alias an input.  d_scratch: at least
 * rtw_denoise_scratch_bytes(w, h) bytes, 16-byte aligned (RTW_EINVAL after the checks above if not); its contents on
 * entry do not matter, and nothing is written beyond that size or beyond d_out's w*h*3 floats. */
int rtw_denoise_device(int device, const float* d_sum, const float* d_sq, const float* d_albedo, const float* d_normal,
                       const float* d_depth, uint32_t w, uint32_t h, uint32_t samples, const uint32_t* d_tile_samples,
                       uint32_t iterations, float sigma_l, float sigma_n, float sigma_z, float* d_out, void* d_scratch,
                       void* stream);
/* The same arithmetic as plain loops over HOST arrays, no GPU (rtw_tonemap's role beside rtw_tonemap_device);
 * RTW_ENOMEM if its work arrays cannot be had. */
int rtw_denoise(const float* rgb_sum, const float* rgb_sq_sum, const float* albedo, const float* normal,
                const float* depth, uint32_t w, uint32_t h, uint32_t samples, const uint32_t* tile_samples,
                uint32_t iterations, float sigma_l, float sigma_n, float sigma_z, float* out);

/* ---- temporal accumulation: the previous frames' accumulated sums, reprojected onto the next camera and added to
 *      the new frame's, so that a sequence of few-sample frames gathers samples over time (SVGF's other half beside
 *      the filter above).  A frame stays what it is everywhere in this library, sums plus counts.  The world is the
 *      same for both frames: motion here lives inside the shutter, so a committed scene is static from frame to frame.
 *      No counterpart in the reference, so the operation is DEFINED here, operation by operation: all arithmetic f32
 *      with one rounding per operation (no fused multiply-add), IEEE division, sqrt and floorf, no transcendentals;
 *      dot(a, b) = (a_0 b_0 + a_1 b_1) + a_2 b_2.  The device kernel, rtw_temporal's host loops and the tests' numpy
 *      restatement agree bit for bit.
 *      An ACCUMULATED FRAME is six full-layout w x h buffers, rows as rtw_render: sum (3 floats per pixel), sq (3),
 *      albedo (3), normal (3), depth (2: the sums of t and of hits), as the render calls leave them, and count
 *      (1 float): the effective samples the other five hold.  A fresh render of n samples is an accumulated frame with
 *      count = (float)n.
 *      Inputs: the CURRENT frame's five sums with `samples` or a tile table (n as for the denoiser) and its camera;
 *      the HISTORY, an accumulated frame and the camera it was rendered with (primed below).  O, llc, H, V, w are a
 *      camera's origin, lower_left_corner, horizontal, vertical and w.
 *      Per pixel p = (i, row), j = h - 1 - row.  "Copy" means: every output is the current value and out_count = c.
 *       1. n = 0: every output, out_count too, is +0.  Otherwise c = (float)n.
 *       2. Copy without a history (hist_count NULL).
 *       3. hits = D_1 (the current depth's second channel).  Copy unless hits > 0.  tbar = D_0 / hits.
 *       4. The world point through the pixel's centre at that depth (the lens offset is ignored: its mean is zero):
 *            s = ((float)i + 0.5f) / (float)(w - 1);  v = ((float)j + 0.5f) / (float)(h - 1);
 *            d_k = ((llc_k + s * H_k) + v * V_k) - O_k;  P_k = O_k + tbar * d_k.
 *       5. Into the history camera:  r_k = P_k - O'_k;  e_k = llc'_k - O'_k;
 *            tau = dot(r, w') / dot(e, w')              (the depth the point would have had in the history frame);
 *            s' = (dot(r, H') / tau - dot(e, H')) / dot(H', H');  v' = (dot(r, V') / tau - dot(e, V')) / dot(V', V');
 *            x = s' * (float)(w - 1) - 0.5f;  y = (float)(h - 1) - (v' * (float)(h - 1) - 0.5f).
 *          Copy unless tau > 0 && x >= -1 && x < (float)w && y >= -1 && y < (float)h (a NaN fails; tested on the floats,
 *          before any conversion to an integer).
 *       6. x0 = floorf(x), fx = x - x0, gx = 1.0f - fx; y0, fy, gy likewise.  Four taps q, in the order (y0, x0),
 *          (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1), with the weights b = gx * gy, fx * gy, gx * fy, fx * fy.
 *          A tap counts iff all of these hold, tested in this order: it is on the image; b > 0; L_q = hist_count[q] > 0;
 *          hq = hist_depth[q]_1 > 0; with zq = hist_depth[q]_0 / hq, fabsf(tau - zq) <= tol_z * tau; with normals
 *          given, dot(g_p, g_q) >= cos_n, g the unit normal of the current / the history normal sum as the denoiser's
 *          prepare makes it (nn = dot(N, N); g_k = nn > 0 ? N_k / sqrtf(nn) : +0); its colour sum is finite:
 *          t = (S_q0 + S_q1) + S_q2, t - t == 0.  Then sb = sb + b, sL = sL + b * L_q and, for every channel of every
 *          buffer in use, sX = sX + b * X_q, all starting at +0, in tap order: the order is the contract.
 *       7. Copy unless sb > 0.  Otherwise Lr = sL / sb;  lam = Lr > max_history ? max_history / Lr : 1.0f;
 *          k = lam / sb;  every output channel is X_cur + k * sX, and out_count = c + k * sL.
 *      So the history enters with at most max_history effective samples (an exponential average once it is reached),
 *      and a pixel the history cannot vouch for -- off the old frame, behind the old camera, disoccluded (the depth
 *      test), on another surface (the normal test) -- starts afresh.  What the definition ignores: the lens offset,
 *      view-dependent shading (a highlight is reprojected as if it stuck to its surface) and geometry that moves.
 *      Buffers: sum, depth, cam, out_sum, out_depth and out_count are required.  sq, albedo and normal are optional
 *      triples (current, history, out): current and out are both given or both NULL, and when they are NULL the
 *      history's is ignored.  hist_count NULL means no history; every other hist pointer and hist_cam are then ignored.
 *      With a history, hist_sum, hist_depth and hist_cam are required, and so is the hist buffer of each triple in use.
 *      An out buffer may be its own current-frame buffer (in place: a pixel reads only its own current values); it may
 *      never be a history buffer, because the call gathers.
 *      Both calls answer RTW_EINVAL for, in this order: a NULL sum, depth, cam, out_sum, out_depth or out_count; a
 *      triple (sq, albedo, normal in turn) given on one side only; with a history, a NULL hist_sum, hist_depth or
 *      hist_cam, then a NULL hist buffer of a triple in use (sq, albedo, normal in turn); with a history, an out buffer
 *      that is a history buffer (equal addresses); an image under 2x2 or over 65536 a side; samples = 0 without a tile
 *      table; max_history NaN, negative or infinite (0 is valid: the history never contributes); tol_z NaN, negative
 *      or infinite; cos_n NaN or outside [-1, 1]. */
/* The pass over DEVICE arrays, enqueued on `stream` (no scene, no scratch: what rtw_tonemap_device is to rtw_tonemap).
 * device < 0 means the current device.  Nothing is written beyond the six out buffers' w*h*(3, 3, 3, 3, 2, 1) floats. */
int rtw_temporal_device(int device, const float* d_sum, const float* d_sq, const float* d_albedo, const float* d_normal,
                        const float* d_depth, uint32_t w, uint32_t h, uint32_t samples, const uint32_t* d_tile_samples,
                        const rtw_camera* cam, const float* d_hist_sum, const float* d_hist_sq,
                        const float* d_hist_albedo, const float* d_hist_normal, const float* d_hist_depth,
                        const float* d_hist_count, const rtw_camera* hist_cam, float max_history, float tol_z,
                        float cos_n, float* d_out_sum, float* d_out_sq, float* d_out_albedo, float* d_out_normal,
                        float* d_out_depth, float* d_out_count, void* stream);
/* The same arithmetic as plain loops over HOST arrays, no GPU. */
int rtw_temporal(const float* rgb_sum, const float* rgb_sq_sum, const float* albedo, const float* normal,
                 const float* depth, uint32_t w, uint32_t h, uint32_t samples, const uint32_t* tile_samples,
                 const rtw_camera* cam, const float* hist_sum, const float* hist_sq, const float* hist_albedo,
                 const float* hist_normal, const float* hist_depth, const float* hist_count,
                 const rtw_camera* hist_cam, float max_history, float tol_z, float cos_n, float* out_sum,
                 float* out_sq, float* out_albedo, float* out_normal, float* out_depth, float* out_count);
/* The denoiser above for an accumulated frame, whose sample count differs per pixel: one change in its prepare.  A
 * pixel's n is count[p] (1 float per pixel); the pixel is empty unless count > 0 (a NaN is empty), and
 * inv = 1.0f / count.  Everything after that is the denoiser's definition, through the same kernels; the same scratch
 * (rtw_denoise_scratch_bytes) and the same checks in the same order, with count among the buffers of the first check
 * and without the one on samples. */
int rtw_denoise_counts_device(int device, const float* d_sum, const float* d_sq, const float* d_albedo,
                              const float* d_normal, const float* d_depth, const float* d_count, uint32_t w,
                              uint32_t h, uint32_t iterations, float sigma_l, float sigma_n, float sigma_z,
                              float* d_out, void* d_scratch, void* stream);
int rtw_denoise_counts(const float* rgb_sum, const float* rgb_sq_sum, const float* albedo, const float* normal,
                       const float* depth, const float* count, uint32_t w, uint32_t h, uint32_t iterations,
                       float sigma_l, float sigma_n, float sigma_z, float* out);

/* ---- closest-hit ray queries: Hittable::hit(&ray, t_min, t_max) -> Option<HitRecord> on the world list
 *      (hittable/mod.rs:22-69) for rays the caller chooses.  A query is world.hit(ray, 0.001, +inf), the interval of
 *      lib.rs:102 and the only one the render's culling is proven for: t_min and t_max are not parameters (the
 *      occlusion queries below take a t_max).  The winner is the render's winner (ties go to the later object; BvhNode
 *      groups are sets), found by the path kernel's own walk for this scene. */
/* ray.rs Ray.  stream: the path RNG state at the segment start, which keys ConstantMedium's free-path sub-stream
 * (rtw_begin_constant_medium); irrelevant for worlds without media.  reserved: 0. */
typedef struct {
  float origin[3], direction[3];
  float time;
  uint32_t reserved;
  uint64_t stream;
} rtw_ray;
/* hittable/mod.rs:22-29 HitRecord.  material: the id the rtw_material_* / rtw_begin_constant_medium call returned.
 * key: the winning leaf's depth-first number in the committed hierarchy, the order rtw_scene_dump lists leaves (a
 * Cuboid counts as its six sides, in rectangular.rs:177-240's order xy, xy, xz, xz, yz, yz; a mesh or
 * rtw_add_triangles call as one leaf per triangle, in input order; a ConstantMedium as one leaf, its boundary not
 * counted).  A miss has flags = 0, t = +inf and zeros elsewhere. */
typedef struct {
  float p[3], normal[3];
  float t, u, v;
  uint32_t material, key, flags;
} rtw_hit;
enum {
  RTW_HIT_HIT = 1,        /* the ray hit: the other fields are the HitRecord */
  RTW_HIT_FRONT_FACE = 2, /* HitRecord::front_face */
  RTW_HIT_BAD_RAY = 4     /* time is NaN or outside the committed motion range: not traced (a miss record) */
};
/* n rays from host memory, blocking: `rays` is rtw_ray[n], `hits` receives rtw_hit[n] (typed void* as `stream` is;
 * the typed forms are in the mirrors).  Rays and records are staged through device buffers the scene's device copy
 * keeps (grown once), at most 2^20 rays at a time, so n is unbounded.  device -1 = the first copy.  RTW_EINVAL: a NULL
 * argument with n > 0, or a ray whose time is NaN or outside the motion range the scene's moving spheres were committed
 * with (found by a host scan before anything is enqueued), or a traversal guard trip (rtw_render_status); RTW_ESTATE:
 * the scene was never flattened by rtw_scene_commit; RTW_ENODEV: no device copy.  n = 0 is RTW_OK and touches no device.
 * Degenerate rays (zero, infinite or NaN components) are legal: the walk is bounded, their records are what the
 * render's arithmetic gives, and their neighbours' records are unaffected.  stats (may be NULL): rays = n, paths = 0,
 * kernel_ms, total_ms; the traversal counters stay 0. */
int rtw_hit_rays(rtw_scene* s, int device, uint64_t n, const void* rays, void* hits, rtw_stats* stats);
/* The same from DEVICE arrays (16-byte aligned) on the caller's `stream`.  It only enqueues unless stats != NULL, as
 * rtw_render_device; a pending guard trip is reported before it enqueues.  No host scan: a ray with a bad time comes
 * back with RTW_HIT_BAD_RAY.  A query uses the device copy's traversal-stack spill area, so queries and renders of one
 * (scene, device) must be serialised on one stream, as renders among themselves (rtw_render_device). */
int rtw_hit_rays_device(rtw_scene* s, int device, uint64_t n, const void* d_rays, void* d_hits, void* stream,
                        rtw_stats* stats);

/* ---- occlusion ray queries: world.hit(&ray, 0.001, t_max).is_some() for rays and bounds the caller chooses (shadow
 *      rays toward a light, ambient occlusion, visibility between two points).  For ray k with bound T = t_max[k]
 *      (+inf for every ray when t_max is NULL), let rec be the record rtw_hit_rays returns for that ray -- the same
 *      walk, the same winner, the same `stream`-keyed media.  Then
 *          occluded[k] = (rec.flags & RTW_HIT_HIT) && !(rec.t > T)
 *      The bound is inclusive: the reference's primitives reject with t > t_max (spherical.rs, rectangular.rs,
 *      triangular.rs, volumes.rs).  A hit whose t is NaN (the in-plane rect hit that only the list-mode loops report)
 *      occludes for every T, as the reference's comparisons let a NaN pass.  T = +inf gives exactly the hit flag;
 *      T < 0.001 gives 0 apart from that NaN case.  So the answer is the reference's world.hit(ray, 0.001, T).is_some(),
 *      with rtw_hit_rays' own deviations only (BvhNode groups as sets).  The kernel builds no record and
 *      does not look for the closest hit: a ray is done at the first hit within T, and boxes beyond T are culled.
 *      A caller t_min is not offered. */
enum {
  RTW_OCCLUDED_HIT = 1,    /* something lies within [0.001, t_max] along the ray */
  RTW_OCCLUDED_BAD_RAY = 2 /* time is NaN or outside the committed motion range, or t_max is NaN: not traced */
};
/* n rays from host memory, blocking: `rays` is rtw_ray[n] exactly as rtw_hit_rays takes it (stream keys media,
 * reserved 0), `t_max` float[n] or NULL, `occluded` receives uint8_t[n]: 0 = free, or RTW_OCCLUDED_HIT.  Rays, bounds
 * and answers are staged through device buffers the scene's device copy keeps, at most 2^20 rays at a time.  device -1
 * = the first copy.  RTW_EINVAL: a NULL argument (the arrays only with n > 0, t_max never), a ray whose time is NaN or
 * outside the committed motion range or whose t_max is NaN (a host scan before anything is enqueued; the message names
 * the ray), or a traversal guard trip; RTW_ESTATE / RTW_ENODEV / n = 0 / degenerate rays as rtw_hit_rays.  Nothing is
 * written beyond n bytes of `occluded`.  stats (may be NULL): rays = n, paths = 0, kernel_ms, total_ms. */
int rtw_occluded_rays(rtw_scene* s, int device, uint64_t n, const void* rays, const float* t_max, uint8_t* occluded,
                      rtw_stats* stats);
/* The same from DEVICE arrays (d_rays 16-byte aligned, d_t_max 4-byte aligned or NULL) on the caller's `stream`; only
 * enqueues unless stats != NULL; a pending guard trip is reported before it enqueues.  No host scan: a ray with a bad
 * time or a NaN t_max comes back RTW_OCCLUDED_BAD_RAY, its neighbours unaffected.  The call uses the device copy's
 * traversal-stack spill area: serialise it on one stream with the renders and queries of the same (scene, device), as
 * rtw_hit_rays_device. */
int rtw_occluded_rays_device(rtw_scene* s, int device, uint64_t n, const void* d_rays, const float* d_t_max,
                             uint8_t* d_occluded, void* stream, rtw_stats* stats);

/* ---- scatter and camera-ray queries: the other half of a caller's own integrator.  Camera::get_ray (camera.rs:66-74)
 *      and Material::scatter + Material::emitted (material.rs:23-26, light_source.rs:17-24) as batch queries over the
 *      committed scene's own material and texture tables, with the render's f32 operations and draw order:
 *      rtw_camera_rays -> (rtw_hit_rays -> rtw_scatter_rays)* reproduces rtw_render's samples bit for bit, with the
 *      same number of rays.  These kernels read only immutable scene tables -- no traversal-stack spill area, path
 *      queue or sample buffer -- so, unlike renders and rtw_hit_rays*, they need not be serialised with the scene's other
 *      work on the device. */
/* material.rs:18-21 Scatter{attenuation, scattered} + Material::emitted: one step of sample_ray after world.hit
 * (lib.rs:102-116) */
typedef struct {
  float attenuation[3]; /* Scatter::attenuation; (1,1,1) for a Dielectric; 0 when not scattered */
  float emitted[3];     /* Material::emitted (DiffuseLight: its texture's value; else 0); a miss: the background */
  uint32_t flags, reserved;
} rtw_scatter;
enum {
  RTW_SCATTER_SCATTERED = 1, /* scatter() returned Some: the out ray is valid, continue with T *= attenuation */
  RTW_SCATTER_MISS = 2,      /* the hit record was a miss: emitted = background (lib.rs:102-105) */
  RTW_SCATTER_BAD = 4        /* not shaded: material id out of range, an RTW_HIT_BAD_RAY record, or stream word 0 */
};
/* The camera rays of paths [first, first + n) of a w x h x spp frame, blocking: `rays` receives rtw_ray[n].  Ray k is
 * path p = first + k in the reference's emission order, the layout of rtw_render's output: with row = h-1-j,
 * p = (row*w + i)*spp + sample.  It is the render's ray for (seed, j, i, sample) -- origin, direction and time per
 * lib.rs:84-86 and camera.rs:66-74 -- and its `stream` is the path's generator state after the time draw, the word the
 * first segment's rtw_hit_rays keys media with and rtw_scatter_rays draws from.  RTW_EINVAL: a NULL argument; an image
 * under 2x2 or a side above 65536; first + n > w*h*spp; a camera shutter outside the committed motion range (the
 * checks of the render calls).  RTW_ESTATE / RTW_ENODEV / n = 0 as rtw_hit_rays.  stats (may be NULL): kernel_ms and
 * total_ms only. */
int rtw_camera_rays(rtw_scene* s, int device, const rtw_camera* cam, uint32_t w, uint32_t h, uint32_t spp,
                    uint64_t seed, uint64_t first, uint64_t n, void* rays, rtw_stats* stats);
/* The same into a DEVICE array (16-byte aligned) on the caller's `stream`; only enqueues unless stats != NULL. */
int rtw_camera_rays_device(rtw_scene* s, int device, const rtw_camera* cam, uint32_t w, uint32_t h, uint32_t spp,
                           uint64_t seed, uint64_t first, uint64_t n, void* d_rays, void* stream, rtw_stats* stats);
/* One shading step for n (ray, hit record) pairs from host memory, blocking: `rays` is rtw_ray[n] and `hits` rtw_hit[n]
 * as rtw_hit_rays consumed and produced them (read: the ray's direction, time and stream; the record's p, normal, u, v,
 * material and flags); `out_rays` receives rtw_ray[n], `out_scatter` rtw_scatter[n].  A scattered ray has origin = p,
 * the material's direction (not normalised), the time kept and `stream` = the generator state after this material's
 * draws: it can be fed straight to the next rtw_hit_rays.  Per record: a miss -> RTW_SCATTER_MISS, emitted =
 * background, the ray copied through; a DiffuseLight -> emitted = its texture at (u, v, p), no flag, no draws, stream
 * unchanged; an absorbed Metal ray -> no flag, emitted 0, stream advanced; a record that cannot be shaded ->
 * RTW_SCATTER_BAD, every other output 0.  out_rays may be `rays` (in place); out_scatter may alias nothing.
 * RTW_EINVAL: a NULL argument with n > 0, or a record whose stream word is 0 (xoroshiro64* never leaves that state;
 * found by a host scan before anything is enqueued).  RTW_ESTATE / RTW_ENODEV / n = 0 / the staging (2^20 records at
 * a time) as rtw_hit_rays.  stats (may be NULL): kernel_ms and total_ms only. */
int rtw_scatter_rays(rtw_scene* s, int device, uint64_t n, const void* rays, const void* hits,
                     const float background[3], void* out_rays, void* out_scatter, rtw_stats* stats);
/* The same over DEVICE arrays (16-byte aligned) on the caller's `stream`; only enqueues unless stats != NULL.  No host
 * scan: a record whose stream word is 0 comes back RTW_SCATTER_BAD. */
int rtw_scatter_rays_device(rtw_scene* s, int device, uint64_t n, const void* d_rays, const void* d_hits,
                            const float background[3], void* d_out_rays, void* d_out_scatter, void* stream,
                            rtw_stats* stats);

/* ---- radiance queries: Raytracer::sample_ray(&ray, rng, depth) -> Color (lib.rs:97-117) for rays the caller chooses
 *      (custom cameras, light probes, irradiance baking, per-sample radiance for the caller's own filters), the whole
 *      path traced on the device in one persistent launch of the scene's own path-kernel variant, with the render's
 *      f32 operations and draw order: the records of a frame's rtw_camera_rays, summed per pixel in sample order, are
 *      rtw_render's image bit for bit, and each record is what the rtw_hit_rays -> rtw_scatter_rays loop gives for
 *      its ray. */
/* lib.rs:97-117 sample_ray for a caller's ray: the render's L = T * terminal */
typedef struct {
  float color[3];     /* sample_ray's value, path_kernel's bits (T*0 for an absorbed / depth-exhausted path) */
  uint32_t segments;  /* world.hit queries this path made (lib.rs:102) */
  uint64_t stream;    /* generator state when the path ended */
  uint32_t flags, reserved;
} rtw_sample;         /* 32 B */
enum { RTW_SAMPLE_END_MISS = 1, RTW_SAMPLE_END_NO_SCATTER = 2 /* light or absorbed */,
       RTW_SAMPLE_BAD_RAY = 4, RTW_SAMPLE_END_DEPTH = 8 };
/* n rays from host memory, blocking: `rays` is rtw_ray[n] as rtw_hit_rays takes it, `samples` receives rtw_sample[n].
 * A ray's `stream` is the path generator's state at the first segment: the materials draw from it and it keys the media
 * sub-streams (rtw_camera_rays' word for a camera ray).  The record's `stream` is the word rtw_scatter_rays' out ray
 * carries at the path's last step: the last segment's own word for a miss or a light, the advanced word for an absorbed
 * Metal ray, the last scattered ray's word when depth ran out.  max_depth = 0: colour +0, segments 0, flags 0, the
 * stream copied through (lib.rs:98-100).  Degenerate rays are legal, as for rtw_hit_rays.  RTW_EINVAL: a NULL argument
 * (the arrays only with n > 0); a ray whose time is NaN or outside the committed motion range, or whose stream word is
 * 0 (a host scan before anything is enqueued); a traversal guard trip.  RTW_ESTATE / RTW_ENODEV / n = 0 / the staging
 * (2^20 rays at a time) as rtw_hit_rays.  stats (may be NULL): rays = the sum of `segments`, counted on the device as
 * a render counts them, paths = n, kernel_ms, total_ms. */
int rtw_sample_rays(rtw_scene* s, int device, uint64_t n, const void* rays, const float background[3],
                    uint32_t max_depth, void* samples, rtw_stats* stats);
/* The same over DEVICE arrays (16-byte aligned) on the caller's `stream`; only enqueues unless stats != NULL; a pending
 * guard trip is reported before it enqueues.  No host scan: a ray with a bad time or a zero stream word comes back with
 * RTW_SAMPLE_BAD_RAY and every other field 0, its neighbours unaffected.  The call uses the device copy's
 * traversal-stack spill area, its counters and its path-id queue: it must be serialised on one stream with the renders
 * and rtw_hit_rays* queries of the same (scene, device), as they among themselves. */
int rtw_sample_rays_device(rtw_scene* s, int device, uint64_t n, const void* d_rays, const float background[3],
                           uint32_t max_depth, void* d_samples, void* stream, rtw_stats* stats);

/* Errors of renders the caller did not wait for. A path kernel whose BVH walk trips its guard (a
 * corrupt tree: the walk is bounded, and the first trip closes the path queue, so the grid drains after
 * about one trip per wave) sets the device's host-mapped error word.  It is reported, and cleared, as
 * RTW_EINVAL by the first rtw_render* call on that device that starts after the faulting render has
 * completed (checked before it enqueues, without waiting: a call made while the faulting kernel still
 * runs passes, and a later one reports it), by rtw_path_kernel_times and any call with stats (both wait
 * first), and by this function, which first waits for all work on the device (hipDeviceSynchronize).
 * RTW_OK = every frame rendered so far on `device` (-1: the first copy) is valid. */
int rtw_render_status(rtw_scene* s, int device);
/* Test hook: overwrite the device copy's first two BVH nodes with a cycle, so that every render of it
 * trips the traversal guard (tests/test_gpu_parity.py).  The scene stays unusable on that device. */
int rtw_diag_corrupt_bvh(rtw_scene* s, int device);
/* Test hook (the multi-device path on a one-GPU node): before rtw_scene_commit, make the scene's devices n
 * LOGICAL devices 0..n-1 that all live on physical device 0.  rtw_scene_commit(s, -1) then uploads n copies,
 * each with its own stream, path queue, sample and packed buffers, so rtw_render_multi(s, n) runs its n > 1
 * path (per-device renders, the grouped send/recv gather to logical device 0, the unpack) on one GPU.  Real
 * RCCL refuses a clique whose ranks share a GPU: pair it with a loopback RCCL through RTW_RCCL_LIB
 * (tests/loopback_rccl).  1 <= n <= 64, else RTW_EINVAL; RTW_ESTATE after the commit. */
int rtw_diag_alias_devices(rtw_scene* s, int n);

/* Raytracer::new(..).render().collect() (lib.rs:40-95) over n_gpus devices of this node, driven from
 * the calling host thread (the reference's Rayon pixel parallelism, lib.rs:57-76, becomes tiles
 * across GPUs).  Tile k goes to device k mod n (rtw_tile_partition); each device renders its tiles
 * on its own stream with its own copy of the scene (commit with device = -1 first); one RCCL gather
 * over xGMI (grouped ncclSend to device 0 / ncclRecv on device 0; librccl.so.1 is opened on first
 * use) brings the tiles to device 0, which assembles the frame and copies it into out_rgb_sum in the
 * same layout as rtw_render.  n_gpus <= 0 = every visible device.  The frame is bit-identical to
 * rtw_render's for every n_gpus (per-pixel random streams).  stats->rays sums the devices,
 * stats->kernel_ms is the slowest device's.  Blocking.  With one device (n_gpus = 1, or 0 on a one-GPU
 * node) it is rtw_render's path on device 0 and never opens RCCL; RTW_RCCL_LIB names another RCCL
 * library to open. */
int rtw_render_multi(rtw_scene* s, int n_gpus, const rtw_camera* cam, const float background[3], uint32_t w,
                     uint32_t h, uint32_t spp, uint32_t max_depth, uint64_t seed, float* out_rgb_sum,
                     rtw_stats* stats);
/* Timing of the scene's last rtw_render_multi call (a scaling run's diagnosis: load imbalance against
 * gather cost): device_ms[d] = device d's render (path kernel + in-order reduction, HIP events on its
 * stream) for d < min(cap, n); *gather_ms (may be NULL) = device 0's stream time from the end of its own
 * render to the arrival of every device's tiles (the RCCL send/recv group, so it includes waiting for the
 * slowest device; 0 for one device).  Returns n (0 before the first call).  Host only, no wait.
 * (No reference counterpart: a benchmark hook beside rtw_render_multi.) */
int rtw_render_multi_times(const rtw_scene* s, float* device_ms, uint32_t cap, float* gather_ms);

/* The frame partition rtw_render_multi (and bench.py's one-process-per-GPU path) uses: the 8x8 tiles
 * of a w x h frame dealt round-robin to n_parts parts; part p gets tiles p, p + n, p + 2n, ...
 * Writes min(cap, ceil(nt / n)) ids (the part's tiles, then padding ids equal to nt, which
 * rtw_unpack_tiles_device skips) and the part's real tile count to *n_ids.  Host only. */
int rtw_tile_partition(uint32_t w, uint32_t h, uint32_t n_parts, uint32_t part, uint32_t* ids, uint32_t cap,
                       uint32_t* n_ids);

/* Scatter packed tiles (as written by rtw_render_device) into a full device image. */
int rtw_unpack_tiles_device(int device, uint32_t w, uint32_t h, const uint32_t* d_tile_ids,
                            uint32_t n_tiles, const float* d_packed, float* d_image, void* stream);

/* Device time (ms, HIP events on the render stream) of the most recent path-kernel launches of
 * rtw_render / rtw_render_device on `device`, oldest first: at most max_n of the last 64, written
 * to ms[]; returns how many (>= 0) or an error, and forgets them.  Waits for those launches, and
 * returns RTW_EINVAL if one of them tripped the traversal guard (rtw_render_status).
 * (Benchmark hook: the render call itself also enqueues the in-order sample reduction.) */
int rtw_path_kernel_times(rtw_scene* s, int device, float* ms, uint32_t max_n);

/* Diagnostics: evaluate the render path's f32 transcendentals on the device over n host values
 * (fn 0 log10f(a), 1 sinf(a), 2 acosf(a), 3 atan2f(a, b); DESIGN.md §Parity: correctly rounded;
 * fn 4 a / b by the camera's Markstein division from the reciprocal RN(1 / b), fn 5 the sphere
 * test's sqrt(a)).
 * Used by the parity tests to pin the device functions against the oracle's. */
int rtw_diag_libm(int fn, uint32_t n, const float* a, const float* b, float* out);
/* Diagnostics: every 32-bit pattern b in [lo, hi] (as a float) through a device fast path, compared bit
 * for bit with the IEEE operation on the device.  fn 0: the render path's reciprocal rcp_rn (v_rcp_f32 +
 * one Newton step) vs 1.0f / b, over |b| in [2^-126, 2^126].  counts[0] = mismatches, counts[1] = patterns
 * outside the fast path's range (skipped); the first min(cap, counts[0]) mismatching patterns go to bad. */
int rtw_diag_sweep(int fn, uint32_t lo, uint32_t hi, uint64_t* counts, uint32_t* bad, uint32_t cap);
/* Diagnostics (host only, no device): the host's RN(1 / b) that the camera's u, v divisions use
 * (rtw_render*: b = w - 1, h - 1), over n values; exact for integer-valued b in [1, 2^24). */
int rtw_diag_recip(uint32_t n, const float* b, float* out);
/* Diagnostics: the per-tile lists a render of (cam, w x h) on `device` builds for its camera rays (the 1024-lane
 * sphere kernel's start ring): per 8x8 tile of the frame, in tile order, 8 words = 16 halfwords, a count
 * and then that many BVH primitive indices in ascending order (halfword 0 = 0xFFFF: more candidates than the cap,
 * knob RTW_TILE_LIST_CAP).  Built whether or not a render of this camera would use them.  records holds cap_words
 * words (>= 8 x tiles); *n_over (may be NULL) = the tiles on overflow; prim_keys (may be NULL) receives the DFS key
 * (rtw_hit::key) of BVH primitive k for k < min(cap_keys, n).  Returns n, the BVH's primitive count, or an error. */
int rtw_diag_tile_lists(rtw_scene* s, int device, const rtw_camera* cam, uint32_t w, uint32_t h, uint32_t* records,
                        uint64_t cap_words, uint32_t* n_over, uint32_t* prim_keys, uint32_t cap_keys);
/* Diagnostics (host only, no device): the lists' beam test (csrc/rtw_tile_beam.h) for one tile of a w x h frame and
 * one box: 1 = a camera ray of the tile may meet the box, 0 = none can, < 0 an error. */
int rtw_diag_tile_beam(const rtw_camera* cam, uint32_t w, uint32_t h, uint32_t tile, const float* box_lo,
                       const float* box_hi);

/* console_app/src/main.rs:68-90 tonemap: sqrt(sum/spp), clamp [0, 0.999], u8(255.999*c). */
int rtw_tonemap(const float* rgb_sum, uint32_t n_pixels, uint32_t spp, uint8_t* rgb8);
/* rtw_tonemap of an adaptive frame: every pixel of 8x8 tile t (row-major tiles, ragged edges whole) with
 * spp = tile_samples[t], byte for byte rtw_tonemap of that tile at that spp; a tile with 0 samples is black.
 * RTW_EINVAL: a NULL buffer, an image under 2x2 or over 65536 a side. */
int rtw_tonemap_tiles(const float* rgb_sum, uint32_t w, uint32_t h, const uint32_t* tile_samples, uint8_t* rgb8);

/* ---- scene presets: console_app/src/scenes.rs restated (jumpy-balls :63-162, two-spheres
 *      :164-209, two-perlin-spheres :211-252, earth :254-288, simple-light :290-348, cornell-box
 *      :350-414, smokey-cornell-box :416-483, book2-final-scene :485-620,
 *      animated-book2-final-scene :622-667, simple-triangle :669-717, wavefront-cow-obj :719-771,
 *      textured-monument :816-858).  `seed` replaces thread_rng() for the random placement;
 *      models_dir holds the meshes and images.  Fills cam (the first camera) and background. */
int rtw_scene_preset(rtw_scene* s, const char* name, float aspect_ratio, uint64_t seed,
                     const char* models_dir, rtw_camera* cam, float background[3]);
/* All cameras of a preset (World = (objects, Vec<Camera>, background), scenes.rs:42-58):
 * 30 for animated-book2-final-scene, 1 otherwise.  *n = the count; min(cap, *n) written. */
int rtw_preset_cameras(const char* name, float aspect_ratio, const char* models_dir, rtw_camera* cams,
                       uint32_t cap, uint32_t* n);

/* Introspection for the test harness: the committed hierarchy as text (DESIGN.md
 * §Scene text).  Returns the required size (incl. NUL) in *needed; writes when cap
 * suffices.  rtw_scene_image(k) returns the k-th image texture's pixels. */
int rtw_scene_dump(const rtw_scene* s, char* buf, size_t cap, size_t* needed);
int rtw_scene_image(const rtw_scene* s, uint32_t k, const uint8_t** rgb8, uint32_t* w, uint32_t* h);
/* 0 leaf primitives, 1 materials, 2 textures, 3 BVH nodes, 4 BVH depth, 5 always-tested
 * primitives, 6 instances, 7 BVH2 nodes, 8 traversal-stack bound, 9 feature mask (rtw_device.hpp
 * Feature; selects the path-kernel variant), 10 Perlin tables, 11 stack bound of the sorted-push
 * walk (LDS-node kernels), 12 runs of the always list (one wrapper chain and one prim kind each: the
 * list-mode rect loop's program), 13 1 if every rect admits the list loop's fast path (|k| < 2^62,
 * ordered bounds), 14 1 if the BVH holds sphere tests (their leaves are padded for origins within D0
 * and farther origins take the far-origin walk), 15 that D0 in thousandths, 16-23 the
 * configuration of the path kernel that the current environment (the RTW_* tuning knobs) selects for this
 * scene (csrc/rtw_path_kernel.hpp KernelCfg): 16 LDS stack rows, 17 1 with the HBM stack spill, 18 waves per
 * SIMD, 19 feature set, 20 workgroup size, 21 node4s of the LDS node table, 22 1 with half-precision
 * nodes, 23 1 for the 16-bit stack over global nodes.  3-23 are valid once rtw_scene_commit has flattened
 * the scene (also when its upload failed for lack of a device). */
int64_t rtw_scene_info(const rtw_scene* s, int what);
/* Introspection for the test harness: the flattened 4-wide BVH (DevNode4, 128 B each, breadth-first
 * numbered; csrc/rtw_device.hpp), valid once rtw_scene_commit has flattened the scene (also when its
 * upload failed for lack of a device).  *nodes points into the scene (read-only, lives as long as it). */
int rtw_scene_nodes(const rtw_scene* s, const void** nodes, uint32_t* n_nodes);
/* The same tree in half precision (DevNode4h, 112 B each: f16 plane offsets from an f16 origin, rounded
 * outward; built when the 16-bit child codes fit, else *n_nodes = 0), as the kernels read it. */
int rtw_scene_nodes_half(const rtw_scene* s, const void** nodes, uint32_t* n_nodes);

#ifdef __cplusplus
}
#endif
#endif
