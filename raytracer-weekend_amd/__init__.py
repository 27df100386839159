"""rtw_amd — Python host mirror of raytracer_weekend_lib's render API over the C-ABI.

The product is ``lib/librtw_amd.so`` (HIP kernels for gfx950 + C++ host, include/rtw.h).
This module is plumbing: ctypes bindings whose names and argument meaning follow the
reference crate (raytracer_weekend_lib/src/), so tests read like the reference's API:

    scene = Scene()
    ground = scene.lambertian(scene.checker(scene.solid_rgb(.2, .3, .1), scene.solid_rgb(.9, .9, .9), 10))
    scene.sphere((0, -1000, 0), 1000, ground)                  # Sphere::new        spherical.rs:79
    with scene.translate((265, 0, 295)), scene.rotate_y(15):   # .rotate_y().translate()
        scene.cuboid((0, 0, 0), (165, 330, 165), white)        # Cuboid::new        rectangular.rs:177
    scene.commit()
    cam = Camera.new((13, 2, 3), (0, 0, 0), (0, 1, 0), 20, 16 / 9, 0.1, 10, 0, 1)   # camera.rs:25
    img, stats = Raytracer(scene, cam, (0.7, 0.8, 1.0), 400, 225, 50).render()       # lib.rs:40-76

There is no CPU fallback: if the shared library is missing this module raises on load,
and without a GPU ``Scene.commit`` raises ``RtwError(-19)``.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
REPO_ROOT = PKG_DIR.parent
LIB_PATH = Path(os.environ.get("RTW_LIB_PATH") or PKG_DIR / "lib" / "librtw_amd.so")  # override: tuning builds
MODELS_DIR = REPO_ROOT / "models"

RTW_EINVAL, RTW_ENOMEM, RTW_ENODEV, RTW_ESTATE, RTW_EIO = -22, -12, -19, -71, -5
FLAG_COUNT_TRAVERSAL = 1
FLAG_FULL_IMAGE = 2  # render_samples_device with tile ids: full-layout sums
NO_MATERIAL = 0xFFFFFFFF


class RtwError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rtw error {code}: {msg}")
        self.code = code


class rtw_camera(C.Structure):  # include/rtw.h, camera.rs:9-20
    _fields_ = [("origin", C.c_float * 3), ("lower_left_corner", C.c_float * 3),
                ("horizontal", C.c_float * 3), ("vertical", C.c_float * 3),
                ("u", C.c_float * 3), ("v", C.c_float * 3), ("w", C.c_float * 3),
                ("lens_radius", C.c_float), ("time0", C.c_float), ("time1", C.c_float)]


class rtw_stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("paths", C.c_uint64), ("kernel_ms", C.c_double),
                ("total_ms", C.c_double), ("node_visits", C.c_uint64), ("prim_tests", C.c_uint64),
                ("prim_tests_by_type", C.c_uint64 * 6), ("simd", C.c_uint64 * 6),
                ("phase_cycles", C.c_uint64 * 4), ("boxes_tested", C.c_uint64), ("sub_cycles", C.c_uint64 * 4)]

    def as_dict(self) -> dict:
        return {"rays": int(self.rays), "paths": int(self.paths), "kernel_ms": float(self.kernel_ms),
                "total_ms": float(self.total_ms), "node_visits": int(self.node_visits),
                "prim_tests": int(self.prim_tests),
                "prim_tests_by_type": [int(x) for x in self.prim_tests_by_type],
                "simd_util": {k: (self.simd[2 * q + 1] / (64.0 * self.simd[2 * q]) if self.simd[2 * q] else None)
                              for q, k in enumerate(("node_loop", "prim_tests", "segments"))},
                "boxes_tested": int(self.boxes_tested),
                "phase_share": dict({k: (self.phase_cycles[q] / self.phase_cycles[3] if self.phase_cycles[3] else None)
                                     for q, k in enumerate(("regen", "trace", "shade"))},
                                    **{k: (self.sub_cycles[q] / self.phase_cycles[3] if self.phase_cycles[3] else None)
                                       for q, k in enumerate(("sample", "node_loop", "leaf_tests", "path_start"))})}


class rtw_pixel(C.Structure):  # lib.rs:120-126 Pixel
    _fields_ = [("row", C.c_uint32), ("column", C.c_uint32), ("color", C.c_float * 3)]


class rtw_progress_msg(C.Structure):  # lib.rs:128-138 ProgressMessage
    _fields_ = [("kind", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("samples_per_pixel", C.c_uint32), ("pixel", rtw_pixel)]


class rtw_ray(C.Structure):  # ray.rs Ray + the segment's stream word (include/rtw.h)
    _fields_ = [("origin", C.c_float * 3), ("direction", C.c_float * 3), ("time", C.c_float),
                ("reserved", C.c_uint32), ("stream", C.c_uint64)]


class rtw_hit(C.Structure):  # hittable/mod.rs:22-29 HitRecord
    _fields_ = [("p", C.c_float * 3), ("normal", C.c_float * 3), ("t", C.c_float), ("u", C.c_float),
                ("v", C.c_float), ("material", C.c_uint32), ("key", C.c_uint32), ("flags", C.c_uint32)]


class rtw_scatter(C.Structure):  # material.rs:18-21 Scatter + Material::emitted (include/rtw.h)
    _fields_ = [("attenuation", C.c_float * 3), ("emitted", C.c_float * 3), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class rtw_sample(C.Structure):  # lib.rs:97-117 sample_ray's value for a caller's ray (include/rtw.h)
    _fields_ = [("color", C.c_float * 3), ("segments", C.c_uint32), ("stream", C.c_uint64), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


HIT_HIT, HIT_FRONT_FACE, HIT_BAD_RAY = 1, 2, 4
OCCLUDED_HIT, OCCLUDED_BAD_RAY = 1, 2
SAMPLE_END_MISS, SAMPLE_END_NO_SCATTER, SAMPLE_BAD_RAY, SAMPLE_END_DEPTH = 1, 2, 4, 8
SAMPLE_DTYPE = np.dtype([("color", np.float32, 3), ("segments", np.uint32), ("stream", np.uint64),
                         ("flags", np.uint32), ("reserved", np.uint32)])
SCATTER_SCATTERED, SCATTER_MISS, SCATTER_BAD = 1, 2, 4
SCATTER_DTYPE = np.dtype([("attenuation", np.float32, 3), ("emitted", np.float32, 3), ("flags", np.uint32),
                          ("reserved", np.uint32)])
RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("direction", np.float32, 3), ("time", np.float32),
                      ("reserved", np.uint32), ("stream", np.uint64)])
HIT_DTYPE = np.dtype([("p", np.float32, 3), ("normal", np.float32, 3), ("t", np.float32), ("u", np.float32),
                      ("v", np.float32), ("material", np.uint32), ("key", np.uint32), ("flags", np.uint32)])
MSG_IMAGE_START, MSG_PIXEL, MSG_IMAGE_END = 0, 1, 2
PIXEL_SINK = C.CFUNCTYPE(C.c_int, C.POINTER(rtw_pixel), C.c_uint32, C.c_void_p)
PIXEL_DTYPE = np.dtype([("row", np.uint32), ("column", np.uint32), ("color", np.float32, 3)])
# rtw_frame_sink: (rgb_sum, rgb_sq_sum, w, h, samples_done, user) -> int
FRAME_SINK = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.c_uint32,
                         C.c_void_p)

_F = C.POINTER(C.c_float)
_U32 = C.POINTER(C.c_uint32)
_U8 = C.POINTER(C.c_uint8)
_SIGS = {
    "rtw_last_error": (C.c_char_p, []),
    "rtw_abi_version": (C.c_int, []),
    "rtw_device_count": (C.c_int, []),
    "rtw_scene_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "rtw_scene_destroy": (None, [C.c_void_p]),
    "rtw_texture_solid": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, _U32]),
    "rtw_texture_checker": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, _U32]),
    "rtw_texture_image": (C.c_int, [C.c_void_p, _U8, C.c_uint32, C.c_uint32, _U32]),
    "rtw_texture_uvdebug": (C.c_int, [C.c_void_p, _U32]),
    "rtw_texture_noise": (C.c_int, [C.c_void_p, _F, _U32, C.c_float, _U32]),
    "rtw_perlin_generate": (C.c_int, [C.c_uint64, _F, _U32]),
    "rtw_material_isotropic": (C.c_int, [C.c_void_p, C.c_uint32, _U32]),
    "rtw_material_lambertian": (C.c_int, [C.c_void_p, C.c_uint32, _U32]),
    "rtw_material_metal": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, _U32]),
    "rtw_material_dielectric": (C.c_int, [C.c_void_p, C.c_float, _U32]),
    "rtw_material_diffuse_light": (C.c_int, [C.c_void_p, C.c_uint32, _U32]),
    "rtw_begin_list": (C.c_int, [C.c_void_p]),
    "rtw_begin_bvh": (C.c_int, [C.c_void_p, C.c_float, C.c_float]),
    "rtw_begin_translate": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float]),
    "rtw_begin_rotate_y": (C.c_int, [C.c_void_p, C.c_float]),
    "rtw_begin_constant_medium": (C.c_int, [C.c_void_p, C.c_float, C.c_uint32, _U32]),
    "rtw_end": (C.c_int, [C.c_void_p]),
    "rtw_add_spheres": (C.c_int, [C.c_void_p, C.c_uint32, _F, _F, _F, _F, _U32]),
    "rtw_add_moving_spheres": (C.c_int, [C.c_void_p, C.c_uint32] + [_F] * 9 + [_U32]),
    "rtw_add_rects": (C.c_int, [C.c_void_p, C.c_uint32, _U32, _F, _F, _F, _F, _F, _U32]),
    "rtw_add_cuboid": (C.c_int, [C.c_void_p, _F, _F, C.c_uint32]),
    "rtw_add_triangles": (C.c_int, [C.c_void_p, C.c_uint32, _F, _F, _U8, _F, _U8, C.c_uint32]),
    "rtw_load_wavefront_obj": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint32, _U32]),
    "rtw_scene_commit": (C.c_int, [C.c_void_p, C.c_int]),
    "rtw_camera_new": (C.c_int, [_F, _F, _F, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                 C.c_float, C.POINTER(rtw_camera)]),
    "rtw_render": (C.c_int, [C.c_void_p, C.POINTER(rtw_camera), _F, C.c_uint32, C.c_uint32, C.c_uint32,
                             C.c_uint32, C.c_uint64, _F, C.POINTER(rtw_stats)]),
    "rtw_render_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(rtw_camera), _F, C.c_uint32, C.c_uint32,
                                    C.c_uint32, C.c_uint32, C.c_uint64, _U32, C.c_uint32, C.c_void_p,
                                    C.c_void_p, C.c_uint32, C.POINTER(rtw_stats)]),
    "rtw_render_device_strided": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(rtw_camera), _F, C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(rtw_stats)]),
    "rtw_render_samples_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(rtw_camera), _F, C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, _U32, C.c_uint32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(rtw_stats)]),
    "rtw_sample_blocks": (C.c_int, [C.c_uint32, C.c_uint32, _U32, _U32, C.c_uint32, _U32]),
    "rtw_render_progressive": (C.c_int, [C.c_void_p, C.POINTER(rtw_camera), _F, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_uint64, C.c_uint32, FRAME_SINK, C.c_void_p,
                                         C.POINTER(rtw_stats)]),
    "rtw_tonemap_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rtw_tile_noise_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                        C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "rtw_render_adaptive_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(rtw_camera), _F, C.c_uint32, C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_float, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.POINTER(rtw_stats)]),
    "rtw_render_adaptive": (C.c_int, [C.c_void_p, C.POINTER(rtw_camera), _F, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_uint32, C.c_uint32, C.c_uint64, C.c_float, _F, _F, _U32, _F,
                                      C.POINTER(rtw_stats)]),
    "rtw_tonemap_tiles_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "rtw_render_features_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(rtw_camera), _F, C.c_uint32, C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_uint64, _U32, C.c_uint32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(rtw_stats)]),
    "rtw_render_features": (C.c_int, [C.c_void_p, C.POINTER(rtw_camera), _F, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_uint64, _F, _F, _F, C.POINTER(rtw_stats)]),
    "rtw_render_ao_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(rtw_camera), C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_uint64, C.c_uint32, C.c_float, _U32, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_uint32, C.POINTER(rtw_stats)]),
    "rtw_render_ao": (C.c_int, [C.c_void_p, C.POINTER(rtw_camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                C.c_uint32, C.c_float, _F, C.POINTER(rtw_stats)]),
    "rtw_denoise_scratch_bytes": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "rtw_denoise_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtw_denoise": (C.c_int, [_F, _F, _F, _F, _F, C.c_uint32, C.c_uint32, C.c_uint32, _U32, C.c_uint32, C.c_float,
                              C.c_float, C.c_float, _F]),
    "rtw_temporal_device": (C.c_int, [C.c_int] + [C.c_void_p] * 5 + [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                      C.POINTER(rtw_camera)] + [C.c_void_p] * 6 + [C.POINTER(rtw_camera), C.c_float,
                                      C.c_float, C.c_float] + [C.c_void_p] * 7),
    "rtw_temporal": (C.c_int, [_F] * 5 + [C.c_uint32, C.c_uint32, C.c_uint32, _U32, C.POINTER(rtw_camera)] + [_F] * 6 +
                               [C.POINTER(rtw_camera), C.c_float, C.c_float, C.c_float] + [_F] * 6),
    "rtw_denoise_counts_device": (C.c_int, [C.c_int] + [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_uint32, C.c_float,
                                            C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtw_denoise_counts": (C.c_int, [_F] * 6 + [C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                     _F]),
    "rtw_hit_rays": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(rtw_ray), C.POINTER(rtw_hit),
                               C.POINTER(rtw_stats)]),
    "rtw_hit_rays_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(rtw_stats)]),
    "rtw_occluded_rays": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(rtw_ray), _F, _U8,
                                    C.POINTER(rtw_stats)]),
    "rtw_occluded_rays_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.POINTER(rtw_stats)]),
    "rtw_camera_rays": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(rtw_camera), C.c_uint32, C.c_uint32, C.c_uint32,
                                  C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(rtw_ray), C.POINTER(rtw_stats)]),
    "rtw_camera_rays_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(rtw_camera), C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                         C.POINTER(rtw_stats)]),
    "rtw_scatter_rays": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(rtw_ray), C.POINTER(rtw_hit), _F,
                                   C.POINTER(rtw_ray), C.POINTER(rtw_scatter), C.POINTER(rtw_stats)]),
    "rtw_scatter_rays_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, _F, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.POINTER(rtw_stats)]),
    "rtw_sample_rays": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(rtw_ray), _F, C.c_uint32,
                                  C.POINTER(rtw_sample), C.POINTER(rtw_stats)]),
    "rtw_sample_rays_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, _F, C.c_uint32, C.c_void_p,
                                         C.c_void_p, C.POINTER(rtw_stats)]),
    "rtw_render_status": (C.c_int, [C.c_void_p, C.c_int]),
    "rtw_diag_corrupt_bvh": (C.c_int, [C.c_void_p, C.c_int]),
    "rtw_diag_alias_devices": (C.c_int, [C.c_void_p, C.c_int]),
    "rtw_path_kernel_times": (C.c_int, [C.c_void_p, C.c_int, _F, C.c_uint32]),
    "rtw_render_multi": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(rtw_camera), _F, C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_uint32, C.c_uint64, _F, C.POINTER(rtw_stats)]),
    "rtw_render_multi_times": (C.c_int, [C.c_void_p, _F, C.c_uint32, _F]),
    "rtw_tile_partition": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _U32, C.c_uint32, _U32]),
    "rtw_render_stream": (C.c_int, [C.c_void_p, C.POINTER(rtw_camera), _F, C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.c_uint32, C.c_uint64, C.c_uint32, PIXEL_SINK, C.c_void_p,
                                    C.POINTER(rtw_stats)]),
    "rtw_progress_encode": (C.c_int, [C.POINTER(rtw_progress_msg), _U8, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rtw_progress_decode": (C.c_int, [_U8, C.c_size_t, C.POINTER(rtw_progress_msg)]),
    "rtw_unpack_tiles_device": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtw_tonemap": (C.c_int, [_F, C.c_uint32, C.c_uint32, _U8]),
    "rtw_tonemap_tiles": (C.c_int, [_F, C.c_uint32, C.c_uint32, _U32, _U8]),
    "rtw_diag_libm": (C.c_int, [C.c_int, C.c_uint32, _F, _F, _F]),
    "rtw_diag_recip": (C.c_int, [C.c_uint32, _F, _F]),
    "rtw_diag_tile_lists": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(rtw_camera), C.c_uint32, C.c_uint32, _U32,
                                      C.c_uint64, _U32, _U32, C.c_uint32]),
    "rtw_diag_tile_beam": (C.c_int, [C.POINTER(rtw_camera), C.c_uint32, C.c_uint32, C.c_uint32, _F, _F]),
    "rtw_diag_sweep": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), _U32, C.c_uint32]),
    "rtw_scene_preset": (C.c_int, [C.c_void_p, C.c_char_p, C.c_float, C.c_uint64, C.c_char_p,
                                   C.POINTER(rtw_camera), _F]),
    "rtw_preset_cameras": (C.c_int, [C.c_char_p, C.c_float, C.c_char_p, C.POINTER(rtw_camera), C.c_uint32,
                                     _U32]),
    "rtw_scene_dump": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rtw_scene_image": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(_U8), _U32, _U32]),
    "rtw_scene_nodes": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _U32]),
    "rtw_scene_nodes_half": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _U32]),
    "rtw_scene_info": (C.c_int64, [C.c_void_p, C.c_int]),
}
EXPORTED_SYMBOLS = tuple(_SIGS)

_lib = None


ABI_VERSION = 7  # include/rtw.h RTW_ABI_VERSION
# the denoiser's starting point (denoise, denoise_device, Raytracer.render_denoised; rtw.hpp and rtw_console use the
# same): DESIGN.md "Denoiser" has the error ratios they give
DENOISE_ITERATIONS, DENOISE_SIGMA_L, DENOISE_SIGMA_N, DENOISE_SIGMA_Z = 5, 4.0, 0.5, 0.1
# temporal accumulation's starting point (temporal, temporal_device, TemporalRenderer; rtw.hpp and rtw_console use the
# same), not a tuned result: the history is capped at max_history = TEMPORAL_MAX_HISTORY_FRAMES * spp effective samples,
# a tap's depth may differ by TEMPORAL_TOL_Z of the reprojected depth, and its normal by arccos(TEMPORAL_COS_N)
TEMPORAL_MAX_HISTORY_FRAMES, TEMPORAL_TOL_Z, TEMPORAL_COS_N = 32, 0.05, 0.9


def lib_sha() -> str:
    """First 16 hex digits of the SHA-256 of the library file this process loads (LIB_PATH): ties profiler
    evidence under profiles/ to the build it was measured on (bench.py attaches it only on a match)."""
    import hashlib
    return hashlib.sha256(LIB_PATH.read_bytes()).hexdigest()[:16] if LIB_PATH.exists() else ""


def lib() -> C.CDLL:
    """Load librtw_amd.so (fails loudly: there is no fallback path)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RtwError(RTW_ENODEV, f"{LIB_PATH} not built (run __graft_entry__.build())")
        # torch-ROCm bundles its own libamdhip64.so.7 + libhsa-runtime64 under the same SONAME as
        # /opt/rocm's; whichever loads first serves the whole process.  Load torch's first so the
        # render core and torch's streams / RCCL share ONE HIP runtime (the other order leaves torch
        # with "No HIP GPUs are available").
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(str(LIB_PATH))
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.rtw_abi_version() != ABI_VERSION:  # rtw_stats layout etc. must match this mirror
            raise RtwError(RTW_ESTATE, f"{LIB_PATH} has ABI {L.rtw_abi_version()}, this mirror {ABI_VERSION}")
        _lib = L
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RtwError(rc, lib().rtw_last_error().decode())


def _fa(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))


def _ua(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint32).reshape(-1))


def _fp(a: np.ndarray):
    return a.ctypes.data_as(_F)


def _up(a: np.ndarray):
    return a.ctypes.data_as(_U32)


def device_count() -> int:
    return int(lib().rtw_device_count())


class Camera:
    """Camera::new (camera.rs:25-64)."""

    def __init__(self, c: rtw_camera):
        self.c = c

    @classmethod
    def new(cls, look_from, look_at, vup, vfov, aspect, aperture, focus_dist, time0=0.0, time1=1.0):
        c = rtw_camera()
        _check(lib().rtw_camera_new(_fp(_fa(look_from)), _fp(_fa(look_at)), _fp(_fa(vup)), vfov, aspect,
                                    aperture, focus_dist, time0, time1, C.byref(c)))
        return cls(c)

    def as_dict(self) -> dict:
        return {k: (list(getattr(self.c, k)) if k not in ("lens_radius", "time0", "time1")
                    else float(getattr(self.c, k))) for k, _ in rtw_camera._fields_}


class Scene:
    """The world: Vec<Box<dyn Hittable>> plus its materials/textures, built by reference
    constructor names (include/rtw.h documents the file:line each one replaces)."""

    def __init__(self):
        p = C.c_void_p()
        _check(lib().rtw_scene_create(C.byref(p)))
        self._p = p
        self._keep = []

    def __del__(self):
        if getattr(self, "_p", None) and _lib is not None:
            _lib.rtw_scene_destroy(self._p)
            self._p = None

    # textures ------------------------------------------------------------
    def _id(self, fn, *args) -> int:
        out = C.c_uint32()
        _check(fn(self._p, *args, C.byref(out)))
        return int(out.value)

    def solid_rgb(self, r, g, b) -> int:
        return self._id(lib().rtw_texture_solid, r, g, b)

    def checker(self, odd: int, even: int, frequency: float) -> int:
        return self._id(lib().rtw_texture_checker, odd, even, frequency)

    def image(self, rgb8: np.ndarray) -> int:
        a = np.ascontiguousarray(rgb8, dtype=np.uint8)
        h, w, _ = a.shape
        return self._id(lib().rtw_texture_image, a.ctypes.data_as(_U8), w, h)

    def uv_debug(self) -> int:
        return self._id(lib().rtw_texture_uvdebug)

    def noise(self, scale: float, perlin=None, seed: int = 0) -> int:
        """Noise::new(Perlin, scale) (texture.rs:83-95).  perlin = (gradients[256, 3],
        permutations[3, 256]); default Perlin::new with the build's seeded stream."""
        g, p = perlin if perlin is not None else perlin_generate(seed)
        g, p = _fa(g), _ua(p)
        return self._id(lib().rtw_texture_noise, _fp(g), _up(p), float(scale))

    # materials -----------------------------------------------------------
    def lambertian(self, tex: int) -> int:
        return self._id(lib().rtw_material_lambertian, tex)

    def lambertian_solid(self, rgb) -> int:
        return self.lambertian(self.solid_rgb(*rgb))

    def metal(self, albedo, fuzz) -> int:
        return self._id(lib().rtw_material_metal, albedo[0], albedo[1], albedo[2], fuzz)

    def dielectric(self, ir) -> int:
        return self._id(lib().rtw_material_dielectric, ir)

    def diffuse_light(self, tex: int) -> int:
        return self._id(lib().rtw_material_diffuse_light, tex)

    def isotropic(self, tex: int) -> int:
        return self._id(lib().rtw_material_isotropic, tex)

    # hierarchy -----------------------------------------------------------
    @contextlib.contextmanager
    def _group(self, rc):
        _check(rc)
        yield self
        _check(lib().rtw_end(self._p))

    def list(self):
        return self._group(lib().rtw_begin_list(self._p))

    def bvh(self, t0=0.0, t1=1.0):
        return self._group(lib().rtw_begin_bvh(self._p, t0, t1))

    def translate(self, offset):
        return self._group(lib().rtw_begin_translate(self._p, *[float(x) for x in offset]))

    def rotate_y(self, degrees):
        return self._group(lib().rtw_begin_rotate_y(self._p, float(degrees)))

    def constant_medium(self, density: float, tex: int):
        """ConstantMedium::new(boundary, density, texture) (volumes.rs:24-35): add the boundary
        (one Sphere or Cuboid, optionally translated / rotated) inside the `with` block."""
        return self._group(lib().rtw_begin_constant_medium(self._p, float(density), tex, None))

    # primitives ----------------------------------------------------------
    def spheres(self, centers, radii, mats) -> None:
        c = np.asarray(centers, np.float32).reshape(-1, 3)
        cx, cy, cz = (_fa(c[:, k]) for k in range(3))
        r, m = _fa(radii), _ua(mats)
        _check(lib().rtw_add_spheres(self._p, len(r), _fp(cx), _fp(cy), _fp(cz), _fp(r), _up(m)))

    def sphere(self, center, radius, mat) -> None:
        self.spheres([center], [radius], [mat])

    def moving_spheres(self, c0, t0, c1, t1, radii, mats) -> None:
        c0 = np.asarray(c0, np.float32).reshape(-1, 3)
        c1 = np.asarray(c1, np.float32).reshape(-1, 3)
        arrs = [_fa(c0[:, 0]), _fa(c0[:, 1]), _fa(c0[:, 2]), _fa(t0), _fa(c1[:, 0]), _fa(c1[:, 1]),
                _fa(c1[:, 2]), _fa(t1), _fa(radii)]
        m = _ua(mats)
        _check(lib().rtw_add_moving_spheres(self._p, len(m), *[_fp(a) for a in arrs], _up(m)))

    def moving_sphere(self, c0, t0, c1, t1, radius, mat) -> None:
        self.moving_spheres([c0], [t0], [c1], [t1], [radius], [mat])

    def rects(self, axis, a0, a1, b0, b1, k, mats) -> None:
        ax = _ua(axis)
        arrs = [_fa(a0), _fa(a1), _fa(b0), _fa(b1), _fa(k)]
        m = _ua(mats)
        _check(lib().rtw_add_rects(self._p, len(m), _up(ax), *[_fp(a) for a in arrs], _up(m)))

    def xy_rect(self, x0, x1, y0, y1, k, mat):
        self.rects([0], [x0], [x1], [y0], [y1], [k], [mat])

    def xz_rect(self, x0, x1, z0, z1, k, mat):
        self.rects([1], [x0], [x1], [z0], [z1], [k], [mat])

    def yz_rect(self, y0, y1, z0, z1, k, mat):
        self.rects([2], [y0], [y1], [z0], [z1], [k], [mat])

    def cuboid(self, p0, p1, mat) -> None:
        _check(lib().rtw_add_cuboid(self._p, _fp(_fa(p0)), _fp(_fa(p1)), mat))

    def triangles(self, verts, mat, normals=None, normal_mask=None, uvs=None, uv_mask=None) -> None:
        v = _fa(verts)
        n = len(v) // 9
        nn = _fa(normals) if normals is not None else None
        uu = _fa(uvs) if uvs is not None else None
        nm = np.ascontiguousarray(normal_mask, np.uint8) if normal_mask is not None else None
        um = np.ascontiguousarray(uv_mask, np.uint8) if uv_mask is not None else None
        _check(lib().rtw_add_triangles(
            self._p, n, _fp(v), _fp(nn) if nn is not None else None,
            nm.ctypes.data_as(_U8) if nm is not None else None, _fp(uu) if uu is not None else None,
            um.ctypes.data_as(_U8) if um is not None else None, mat))

    def load_wavefront_obj(self, path, material_override: int = NO_MATERIAL) -> int:
        n = C.c_uint32()
        _check(lib().rtw_load_wavefront_obj(self._p, str(path).encode(), None, material_override, C.byref(n)))
        return int(n.value)

    def preset(self, name: str, aspect: float, seed: int = 0, models_dir=None):
        """console_app/src/scenes.rs scene by subcommand name -> (Camera, background)."""
        cam = rtw_camera()
        bg = np.zeros(3, np.float32)
        md = str(models_dir or MODELS_DIR).encode()
        _check(lib().rtw_scene_preset(self._p, name.encode(), aspect, seed, md, C.byref(cam), _fp(bg)))
        return Camera(cam), tuple(float(x) for x in bg)

    def commit(self, device: int = -1) -> "Scene":
        _check(lib().rtw_scene_commit(self._p, device))
        return self

    # introspection -------------------------------------------------------
    def dump(self) -> str:
        need = C.c_size_t()
        _check(lib().rtw_scene_dump(self._p, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        _check(lib().rtw_scene_dump(self._p, buf, need.value, C.byref(need)))
        return buf.value.decode()

    def images(self) -> list:
        out, k = [], 0
        while True:
            px, w, h = _U8(), C.c_uint32(), C.c_uint32()
            if lib().rtw_scene_image(self._p, k, C.byref(px), C.byref(w), C.byref(h)) != 0:
                return out
            out.append(np.ctypeslib.as_array(px, shape=(h.value * w.value * 3,)).copy())
            k += 1

    def path_kernel_times(self, device: int = -1, max_n: int = 64) -> list:
        """Device ms of the recent path-kernel launches on `device` (oldest first; waits for them)."""
        buf = (C.c_float * max_n)()
        n = lib().rtw_path_kernel_times(self._p, device, buf, max_n)
        if n < 0:
            _check(n)
        return [float(buf[q]) for q in range(n)]

    def multi_times(self, max_n: int = 64):
        """(per-device render ms, device 0's gather ms) of the last rtw_render_multi call on this scene."""
        buf, g = (C.c_float * max_n)(), C.c_float()
        n = lib().rtw_render_multi_times(self._p, buf, max_n, C.byref(g))
        if n < 0:
            _check(n)
        return [float(buf[q]) for q in range(min(n, max_n))], float(g.value)

    def hit_rays(self, origins, directions, times=None, streams=None, device: int = -1, want_stats: bool = False):
        """world.hit(ray, 0.001, inf) (hittable/mod.rs:57-69) for n rays: origins and directions [n, 3], times [n]
        (default 0) and the segments' stream words [n] (default 0; they key a ConstantMedium's free path).
        -> records as a structured array of HIT_DTYPE (rtw_hit's layout)[, stats]."""
        rays = make_rays(origins, directions, times, streams)
        hits = np.zeros(len(rays), HIT_DTYPE)
        st = rtw_stats()
        _check(lib().rtw_hit_rays(self._p, device, len(rays), rays.ctypes.data_as(C.POINTER(rtw_ray)),
                                  hits.ctypes.data_as(C.POINTER(rtw_hit)), C.byref(st)))
        return (hits, st.as_dict()) if want_stats else hits

    def hit_rays_device(self, d_rays_ptr: int, d_hits_ptr: int, n: int, device: int = 0, stream_ptr: int = 0,
                        want_stats: bool = False):
        """Enqueue the query of n rays in device memory (rtw_ray[n] -> rtw_hit[n], both 16-byte aligned) on a
        stream; waits only for stats."""
        st = rtw_stats()
        _check(lib().rtw_hit_rays_device(self._p, device, n, C.c_void_p(d_rays_ptr), C.c_void_p(d_hits_ptr),
                                         C.c_void_p(stream_ptr), C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def occluded_rays(self, origin, direction, time=None, stream=None, t_max=None, device: int = 0,
                      want_stats: bool = False):
        """world.hit(ray, 0.001, t_max).is_some() for n rays given as hit_rays takes them, t_max [n] or None (+inf):
        rtw_hit_rays' record with `hit and not t > t_max`, the bound inclusive, found by an any-hit walk.
        -> a uint8 array [n]: 0 = free, OCCLUDED_HIT[, stats]."""
        rays = make_rays(origin, direction, time, stream)
        out = np.zeros(len(rays), np.uint8)
        tm = None
        if t_max is not None:
            tm = np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, np.float32), (len(rays),)))
        st = rtw_stats()
        _check(lib().rtw_occluded_rays(self._p, device, len(rays), rays.ctypes.data_as(C.POINTER(rtw_ray)),
                                       tm.ctypes.data_as(_F) if tm is not None else None, out.ctypes.data_as(_U8),
                                       C.byref(st)))
        return (out, st.as_dict()) if want_stats else out

    def occluded_rays_device(self, d_rays_ptr: int, d_t_max_ptr: int, d_out_ptr: int, n: int, device: int = 0,
                             stream_ptr: int = 0, want_stats: bool = False):
        """Enqueue the query of n rays in device memory (rtw_ray[n], 16-byte aligned; float[n] or 0; -> uint8[n]) on a
        stream; waits only for stats.  A bad time or a NaN t_max comes back OCCLUDED_BAD_RAY."""
        st = rtw_stats()
        _check(lib().rtw_occluded_rays_device(self._p, device, n, C.c_void_p(d_rays_ptr), C.c_void_p(d_t_max_ptr or None),
                                              C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr),
                                              C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def camera_rays(self, cam: "Camera", w: int, h: int, spp: int, seed: int, first: int = 0, n=None,
                    device: int = -1, want_stats: bool = False):
        """Camera::get_ray as the render calls it (lib.rs:84-86, camera.rs:66-74): the rays of paths [first, first + n)
        of a w x h x spp frame in rtw_render's output order, p = ((h-1-j)*w + i)*spp + sample (n = None: to the
        frame's end), each with its path's stream word after the camera's draws.  -> RAY_DTYPE records[, stats]."""
        n = w * h * spp - first if n is None else n
        rays = np.zeros(max(n, 0), RAY_DTYPE)
        st = rtw_stats()
        _check(lib().rtw_camera_rays(self._p, device, C.byref(cam.c), w, h, spp, seed, first, n,
                                     rays.ctypes.data_as(C.POINTER(rtw_ray)), C.byref(st)))
        return (rays, st.as_dict()) if want_stats else rays

    def camera_rays_device(self, cam: "Camera", w: int, h: int, spp: int, seed: int, first: int, n: int,
                           d_rays_ptr: int, device: int = 0, stream_ptr: int = 0, want_stats: bool = False):
        """Enqueue the same into device memory (rtw_ray[n], 16-byte aligned) on a stream; waits only for stats."""
        st = rtw_stats()
        _check(lib().rtw_camera_rays_device(self._p, device, C.byref(cam.c), w, h, spp, seed, first, n,
                                            C.c_void_p(d_rays_ptr), C.c_void_p(stream_ptr),
                                            C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def scatter_rays(self, rays, hits, background, device: int = -1, want_stats: bool = False):
        """Material::scatter + Material::emitted (material.rs:23-26, light_source.rs:17-24; a miss: the background,
        lib.rs:102-105) for RAY_DTYPE rays and the HIT_DTYPE records hit_rays gave for them.
        -> (out_rays as RAY_DTYPE, scatter as SCATTER_DTYPE)[, stats]."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        hits = np.ascontiguousarray(hits, HIT_DTYPE)
        if len(rays) != len(hits):
            raise ValueError("rays and hits differ in length")
        out = np.zeros(len(rays), RAY_DTYPE)
        sc = np.zeros(len(rays), SCATTER_DTYPE)
        st = rtw_stats()
        _check(lib().rtw_scatter_rays(self._p, device, len(rays), rays.ctypes.data_as(C.POINTER(rtw_ray)),
                                      hits.ctypes.data_as(C.POINTER(rtw_hit)), _fp(_fa(background)),
                                      out.ctypes.data_as(C.POINTER(rtw_ray)),
                                      sc.ctypes.data_as(C.POINTER(rtw_scatter)), C.byref(st)))
        return (out, sc, st.as_dict()) if want_stats else (out, sc)

    def scatter_rays_device(self, d_rays_ptr: int, d_hits_ptr: int, background, d_out_rays_ptr: int,
                            d_out_scatter_ptr: int, n: int, device: int = 0, stream_ptr: int = 0,
                            want_stats: bool = False):
        """Enqueue the same over device arrays (16-byte aligned; d_out_rays_ptr may be d_rays_ptr) on a stream; waits
        only for stats."""
        st = rtw_stats()
        _check(lib().rtw_scatter_rays_device(self._p, device, n, C.c_void_p(d_rays_ptr), C.c_void_p(d_hits_ptr),
                                             _fp(_fa(background)), C.c_void_p(d_out_rays_ptr),
                                             C.c_void_p(d_out_scatter_ptr), C.c_void_p(stream_ptr),
                                             C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def sample_rays(self, rays, background, max_depth: int = 50, device: int = -1, want_stats: bool = False):
        """Raytracer::sample_ray (lib.rs:97-117) for RAY_DTYPE rays the caller chose (make_rays, camera_rays): every
        path traced to its end on the device in one launch, with the render's arithmetic and draw order.  A ray's
        stream word (non-zero) is its path's generator state.  -> SAMPLE_DTYPE records (color, segments, the final
        stream word, SAMPLE_END_* flags)[, stats: rays = the segments traced, paths = n]."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        out = np.zeros(len(rays), SAMPLE_DTYPE)
        st = rtw_stats()
        _check(lib().rtw_sample_rays(self._p, device, len(rays), rays.ctypes.data_as(C.POINTER(rtw_ray)),
                                     _fp(_fa(background)), max_depth, out.ctypes.data_as(C.POINTER(rtw_sample)),
                                     C.byref(st)))
        return (out, st.as_dict()) if want_stats else out

    def sample_rays_device(self, d_rays_ptr: int, background, max_depth: int, d_samples_ptr: int, n: int,
                           device: int = 0, stream_ptr: int = 0, want_stats: bool = False):
        """Enqueue the same over device arrays (rtw_ray[n] -> rtw_sample[n], 16-byte aligned) on a stream, which must
        be the one the scene's renders and hit queries run on; waits only for stats."""
        st = rtw_stats()
        _check(lib().rtw_sample_rays_device(self._p, device, n, C.c_void_p(d_rays_ptr), _fp(_fa(background)),
                                            max_depth, C.c_void_p(d_samples_ptr), C.c_void_p(stream_ptr),
                                            C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def render_status(self, device: int = -1) -> None:
        """Wait for the device and raise if a render since the last check tripped the traversal guard."""
        _check(lib().rtw_render_status(self._p, device))

    def diag_corrupt_bvh(self, device: int = -1) -> None:
        """Test hook: a cyclic BVH on the device copy (every render of it trips the guard)."""
        _check(lib().rtw_diag_corrupt_bvh(self._p, device))

    def diag_alias_devices(self, n: int) -> "Scene":
        """Test hook (before commit): n logical devices on physical device 0, so rtw_render_multi's n > 1
        path runs on one GPU (with the loopback RCCL of tests/loopback_rccl via RTW_RCCL_LIB)."""
        _check(lib().rtw_diag_alias_devices(self._p, int(n)))
        return self

    def info(self, what: int) -> int:
        return int(lib().rtw_scene_info(self._p, what))

    def nodes(self) -> np.ndarray:
        """The flattened BVH4 (DevNode4 records, rtw_device.hpp) as a structured array (a copy)."""
        p, n = C.c_void_p(), C.c_uint32()
        _check(lib().rtw_scene_nodes(self._p, C.byref(p), C.byref(n)))
        dt = np.dtype([("lo_x", "<f4", 4), ("hi_x", "<f4", 4), ("lo_y", "<f4", 4), ("hi_y", "<f4", 4),
                       ("lo_z", "<f4", 4), ("hi_z", "<f4", 4), ("child", "<i4", 4), ("code", "<u4", 4)])
        if not n.value:
            return np.zeros(0, dt)
        buf = (C.c_uint8 * (128 * n.value)).from_address(p.value)
        return np.frombuffer(bytes(buf), dtype=dt).copy()


    def nodes_half(self) -> np.ndarray:
        """The half-precision BVH4 (DevNode4h, rtw_device.hpp) as a structured array (a copy; empty when
        the 16-bit codes do not fit).  Planes are f16 offsets from `origin`: x[0] = lo x4, hi x4 and x[1] =
        hi x4, lo x4 (likewise y, z)."""
        p, n = C.c_void_p(), C.c_uint32()
        _check(lib().rtw_scene_nodes_half(self._p, C.byref(p), C.byref(n)))
        dt = np.dtype([("x", "<f2", (2, 8)), ("y", "<f2", (2, 8)), ("z", "<f2", (2, 8)), ("code", "<u2", 4),
                       ("origin", "<f2", 3), ("pad", "<u2")])
        assert dt.itemsize == 112
        if not n.value:
            return np.zeros(0, dt)
        buf = (C.c_uint8 * (112 * n.value)).from_address(p.value)
        return np.frombuffer(bytes(buf), dtype=dt).copy()


class Raytracer:
    """Raytracer::new(world, cam, background, w, h, spp) (lib.rs:40-48) + render() (:57-95)."""

    def __init__(self, scene: Scene, cam: Camera, background, image_width: int, image_height: int,
                 samples_per_pixel: int, seed: int = 0, max_depth: int = 50):
        self.scene, self.cam = scene, cam
        self.bg = _fa(background)
        self.w, self.h, self.spp = int(image_width), int(image_height), int(samples_per_pixel)
        self.seed, self.max_depth = int(seed), int(max_depth)

    def render(self):
        """-> (sums[h, w, 3] float32 in reference emission order: row r is j = h-1-r, stats)."""
        out = np.empty((self.h, self.w, 3), np.float32)
        st = rtw_stats()
        _check(lib().rtw_render(self.scene._p, C.byref(self.cam.c), _fp(self.bg), self.w, self.h, self.spp,
                                self.max_depth, self.seed, out.ctypes.data_as(_F), C.byref(st)))
        return out, st.as_dict()

    def render_multi(self, n_gpus: int = 0):
        """The same frame over n_gpus devices from this thread (rtw_render_multi: interleaved tiles,
        one RCCL gather to device 0); n_gpus <= 0 = every visible device.  -> (sums, stats)."""
        out = np.empty((self.h, self.w, 3), np.float32)
        st = rtw_stats()
        _check(lib().rtw_render_multi(self.scene._p, int(n_gpus), C.byref(self.cam.c), _fp(self.bg), self.w, self.h,
                                      self.spp, self.max_depth, self.seed, out.ctypes.data_as(_F), C.byref(st)))
        return out, st.as_dict()

    def render_stream(self, on_pixels, band_rows: int = 64):
        """Raytracer::render() as a progressive Pixel stream (lib.rs:50-76): on_pixels(array of
        PIXEL_DTYPE records) per finished band, in emission order (row j = h-1 .. 0).  -> stats."""
        err = []

        def sink(px, n, _user):
            try:
                buf = C.string_at(px, n * C.sizeof(rtw_pixel))
                on_pixels(np.frombuffer(buf, PIXEL_DTYPE).copy())
                return 0
            except Exception as e:  # stop the render, re-raise below
                err.append(e)
                return RTW_ESTATE

        cb = PIXEL_SINK(sink)
        st = rtw_stats()
        rc = lib().rtw_render_stream(self.scene._p, C.byref(self.cam.c), _fp(self.bg), self.w, self.h, self.spp,
                                     self.max_depth, self.seed, band_rows, cb, None, C.byref(st))
        if err:
            raise err[0]
        _check(rc)
        return st.as_dict()

    def render_device(self, d_out_ptr: int, device: int = 0, d_tiles_ptr: int = 0, n_tiles: int = 0,
                      stream_ptr: int = 0, flags: int = 0, want_stats: bool = False):
        """Enqueue into device memory.  d_tiles_ptr: device uint32 tile ids (0 = whole image,
        full-layout output); with tiles the output is packed [n_tiles][64][3]."""
        st = rtw_stats()
        _check(lib().rtw_render_device(
            self.scene._p, device, C.byref(self.cam.c), _fp(self.bg), self.w, self.h, self.spp, self.max_depth,
            self.seed, C.cast(C.c_void_p(d_tiles_ptr), _U32) if d_tiles_ptr else None, n_tiles,
            C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr), flags, C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def render_device_strided(self, d_out_ptr: int, device: int, first_tile: int, tile_stride: int, n_tiles: int,
                              stream_ptr: int = 0, flags: int = 0, want_stats: bool = False):
        """Enqueue tiles first_tile + k * tile_stride (k < n_tiles) into packed device memory
        [n_tiles][64][3] (a device's round-robin share of the frame, no id table)."""
        st = rtw_stats()
        _check(lib().rtw_render_device_strided(
            self.scene._p, device, C.byref(self.cam.c), _fp(self.bg), self.w, self.h, self.spp, self.max_depth,
            self.seed, first_tile, tile_stride, n_tiles, C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr), flags,
            C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None


    def render_samples_device(self, d_sum_ptr: int, d_sq_ptr: int = 0, sample_first: int = 0, n_samples=None,
                              device: int = 0, d_tiles_ptr: int = 0, n_tiles: int = 0, stream_ptr: int = 0,
                              flags: int = 0, want_stats: bool = False):
        """Enqueue samples [sample_first, sample_first + n_samples) (n_samples = None: up to the frame's spp), ADDED in
        sample order onto the device sums at d_sum_ptr and, unless 0, the sums of squares at d_sq_ptr (zeroed buffers =
        a fresh frame); tiles and layouts as render_device.  Chunks that cover [0, spp) give render()'s frame bit for
        bit."""
        n = max(self.spp - sample_first, 0) if n_samples is None else n_samples
        st = rtw_stats()
        _check(lib().rtw_render_samples_device(
            self.scene._p, device, C.byref(self.cam.c), _fp(self.bg), self.w, self.h, sample_first, n, self.max_depth,
            self.seed, C.cast(C.c_void_p(d_tiles_ptr), _U32) if d_tiles_ptr else None, n_tiles,
            C.c_void_p(d_sum_ptr), C.c_void_p(d_sq_ptr) if d_sq_ptr else None, C.c_void_p(stream_ptr), flags,
            C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def render_progressive(self, on_frame, step: int = 0):
        """The frame in growing steps (rtw_render_progressive: they end at 1, 2, 4, ... samples while the doubled count
        is within `step`, then every `step` samples; 0 = doubling, then spp): on_frame(sums[h, w, 3], sums of
        squares[h, w, 3], samples_done) after each, on copies it may keep.  A return value that is true as an int
        stops the render.  -> (that value, or 0 after the last step; stats: totals over the call)."""
        err = []
        shape = (self.h, self.w, 3)

        def sink(p_sum, p_sq, _w, _h, done, _user):
            try:
                a = np.ctypeslib.as_array(p_sum, shape=shape).copy()
                b = np.ctypeslib.as_array(p_sq, shape=shape).copy()
                return int(on_frame(a, b, int(done)) or 0)
            except Exception as e:  # stop the render, re-raise below
                err.append(e)
                return RTW_ESTATE

        cb = FRAME_SINK(sink)
        st = rtw_stats()
        rc = lib().rtw_render_progressive(self.scene._p, C.byref(self.cam.c), _fp(self.bg), self.w, self.h, self.spp,
                                          self.max_depth, self.seed, step, cb, None, C.byref(st))
        if err:
            raise err[0]
        if rc < 0:
            _check(rc)
        return rc, st.as_dict()


    def render_adaptive(self, threshold: float, min_spp: int = 16, want_sq: bool = False):
        """The frame with a sample count per 8x8 tile (rtw_render_adaptive; the constructor's spp is the maximum): rounds
        end at min_spp, 2 min_spp, ... samples, and a tile stops once its noise estimate is <= threshold.  A tile that
        stopped at n samples holds render()'s pixels of an n-spp frame.  -> (sums[h, w, 3], tile_samples[tiles],
        tile_err[tiles], stats), with the sums of squares[h, w, 3] after the sums when want_sq."""
        out = np.empty((self.h, self.w, 3), np.float32)
        sq = np.empty((self.h, self.w, 3), np.float32) if want_sq else None
        nt = n_tiles(self.w, self.h)
        ts, err = np.zeros(nt, np.uint32), np.zeros(nt, np.float32)
        st = rtw_stats()
        _check(lib().rtw_render_adaptive(self.scene._p, C.byref(self.cam.c), _fp(self.bg), self.w, self.h, min_spp,
                                         self.spp, self.max_depth, self.seed, threshold, _fp(out),
                                         _fp(sq) if want_sq else None, _up(ts), _fp(err), C.byref(st)))
        return (out, sq, ts, err, st.as_dict()) if want_sq else (out, ts, err, st.as_dict())

    def render_adaptive_device(self, threshold: float, d_sum_ptr: int, d_sq_ptr: int, d_tile_samples_ptr: int,
                               d_tile_err_ptr: int = 0, min_spp: int = 16, device: int = 0, stream_ptr: int = 0,
                               flags: int = 0, want_stats: bool = False):
        """render_adaptive into device memory (rtw_render_adaptive_device; blocking on the stream): full-layout sums and
        sums of squares (zeroed by the call), tile_samples[tiles] (uint32) and, unless 0, tile_err[tiles] (float32)."""
        st = rtw_stats()
        _check(lib().rtw_render_adaptive_device(
            self.scene._p, device, C.byref(self.cam.c), _fp(self.bg), self.w, self.h, min_spp, self.spp, self.max_depth,
            self.seed, threshold, C.c_void_p(d_sum_ptr), C.c_void_p(d_sq_ptr), C.c_void_p(d_tile_samples_ptr),
            C.c_void_p(d_tile_err_ptr) if d_tile_err_ptr else None, C.c_void_p(stream_ptr), flags,
            C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def render_features(self, want=("albedo", "normal", "depth")):
        """The denoiser's guides for this frame (rtw_render_features): per pixel the sums over its spp camera rays of the
        first hit's albedo[h, w, 3], normal[h, w, 3] and depth[h, w, 2] = (t, 1) (the background, +0 and (0, 0) for a
        miss; the second depth channel is the hit count), in render()'s row order.  Sample s is render()'s camera ray s.
        -> ({name: array for the names in `want`}, stats)."""
        names = ("albedo", "normal", "depth")
        bad = [n for n in want if n not in names]
        if bad:
            raise ValueError(f"unknown feature buffers {bad}: {names}")
        out = {n: np.empty((self.h, self.w, 2 if n == "depth" else 3), np.float32) for n in names if n in want}
        st = rtw_stats()
        _check(lib().rtw_render_features(self.scene._p, C.byref(self.cam.c), _fp(self.bg), self.w, self.h, self.spp,
                                         self.seed, *[_fp(out[n]) if n in out else None for n in names], C.byref(st)))
        return out, st.as_dict()

    def render_features_device(self, d_albedo_ptr: int = 0, d_normal_ptr: int = 0, d_depth_ptr: int = 0,
                               sample_first: int = 0, n_samples=None, device: int = 0, d_tiles_ptr: int = 0,
                               n_tiles: int = 0, stream_ptr: int = 0, flags: int = 0, want_stats: bool = False):
        """Enqueue the features of samples [sample_first, sample_first + n_samples) (n_samples = None: up to the frame's
        spp), ADDED in sample order onto the device sums (3, 3 and 2 floats per pixel; 0 = not wanted, not all three);
        tiles, layouts and flags as render_samples_device.  Chunks that cover [0, spp) give render_features()' buffers
        bit for bit."""
        n = max(self.spp - sample_first, 0) if n_samples is None else n_samples
        st = rtw_stats()
        _check(lib().rtw_render_features_device(
            self.scene._p, device, C.byref(self.cam.c), _fp(self.bg), self.w, self.h, sample_first, n, self.seed,
            C.cast(C.c_void_p(d_tiles_ptr), _U32) if d_tiles_ptr else None, n_tiles,
            C.c_void_p(d_albedo_ptr) if d_albedo_ptr else None, C.c_void_p(d_normal_ptr) if d_normal_ptr else None,
            C.c_void_p(d_depth_ptr) if d_depth_ptr else None, C.c_void_p(stream_ptr), flags,
            C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def render_ao(self, ao_rays: int = 1, radius: float = float("inf")):
        """The ambient-occlusion buffer of this frame (rtw_render_ao; include/rtw.h defines it): per pixel the sums over
        its spp camera rays of (open, cast) -- of the ao_rays Lambertian-distributed rays cast from each first hit, those
        that reach `radius` unoccluded, and those cast (a miss casts none).  radius = inf: sky visibility.  Mean AO =
        open / cast.  -> (ao[h, w, 2] in render()'s row order, stats: paths = camera samples, rays = paths + AO rays)."""
        out = np.empty((self.h, self.w, 2), np.float32)
        st = rtw_stats()
        _check(lib().rtw_render_ao(self.scene._p, C.byref(self.cam.c), self.w, self.h, self.spp, self.seed, ao_rays,
                                   radius, _fp(out), C.byref(st)))
        return out, st.as_dict()

    def render_denoised(self, iterations: int = DENOISE_ITERATIONS, sigma_l: float = DENOISE_SIGMA_L,
                        sigma_n: float = DENOISE_SIGMA_N, sigma_z: float = DENOISE_SIGMA_Z, device: int = 0):
        """The frame at its spp, denoised on the device: render_samples_device with the sums of squares, then
        render_features_device, then denoise_device, on device buffers this object keeps from one call to the next
        (torch tensors on cuda:device), default stream.  -> (mean radiance[h, w, 3] in render()'s row order, stats of
        the colour samples)."""
        import torch

        px = self.w * self.h
        key = (device, self.w, self.h)
        if getattr(self, "_denoise_key", None) != key:
            dev = torch.device("cuda", device)
            self._denoise_bufs = (torch.empty(px * 14, dtype=torch.float32, device=dev),
                                  torch.empty(denoise_scratch_bytes(self.w, self.h), dtype=torch.uint8, device=dev),
                                  torch.empty(px * 3, dtype=torch.float32, device=dev))
            self._denoise_key = key
        sums, scratch, out = self._denoise_bufs
        sums.zero_()
        torch.cuda.synchronize(device)
        b = sums.data_ptr()
        d_sum, d_sq, d_alb, d_nrm, d_dep = (b + 4 * px * k for k in (0, 3, 6, 9, 12))
        st = self.render_samples_device(d_sum, d_sq, device=device, want_stats=True)
        self.render_features_device(d_alb, d_nrm, d_dep, device=device)
        denoise_device(d_sum, d_sq, d_alb, d_nrm, d_dep, self.w, self.h, self.spp, out.data_ptr(), scratch.data_ptr(),
                       iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_z=sigma_z, device=device)
        torch.cuda.synchronize(device)
        return out.cpu().numpy().reshape(self.h, self.w, 3), st


def render_ao_device(scene: "Scene", cam: "Camera", w: int, h: int, d_ao_ptr: int, n_samples: int, ao_rays: int = 1,
                     radius: float = float("inf"), seed: int = 0, sample_first: int = 0, device: int = 0,
                     d_tiles_ptr: int = 0, n_tiles: int = 0, stream_ptr: int = 0, flags: int = 0,
                     want_stats: bool = False):
    """rtw_render_ao_device: enqueue the ambient occlusion of samples [sample_first, sample_first + n_samples), ADDED in
    sample order onto the device sums at d_ao_ptr (2 floats per pixel: open, cast; zeroed = a fresh frame); tiles,
    layouts, stream and flags as Raytracer.render_features_device.  Chunks that cover [0, spp) give
    Raytracer.render_ao()'s buffer bit for bit.  -> stats with want_stats (then the call waits), else None."""
    st = rtw_stats()
    _check(lib().rtw_render_ao_device(
        scene._p, device, C.byref(cam.c), w, h, sample_first, n_samples, seed, ao_rays, radius,
        C.cast(C.c_void_p(d_tiles_ptr), _U32) if d_tiles_ptr else None, n_tiles,
        C.c_void_p(d_ao_ptr) if d_ao_ptr else None, C.c_void_p(stream_ptr), flags,
        C.byref(st) if want_stats else None))
    return st.as_dict() if want_stats else None


def denoise_scratch_bytes(w: int, h: int) -> int:
    """rtw_denoise_scratch_bytes: the device scratch denoise_device needs for a w x h image (host only)."""
    n = C.c_uint64()
    _check(lib().rtw_denoise_scratch_bytes(w, h, C.byref(n)))
    return int(n.value)


def denoise_device(d_sum_ptr: int, d_sq_ptr: int, d_albedo_ptr: int, d_normal_ptr: int, d_depth_ptr: int, w: int,
                   h: int, samples: int, d_out_ptr: int, d_scratch_ptr: int, d_tile_samples_ptr: int = 0,
                   iterations: int = DENOISE_ITERATIONS, sigma_l: float = DENOISE_SIGMA_L,
                   sigma_n: float = DENOISE_SIGMA_N, sigma_z: float = DENOISE_SIGMA_Z, device: int = -1,
                   stream_ptr: int = 0):
    """rtw_denoise_device: enqueue the edge-avoiding a-trous filter (include/rtw.h defines it) over full-layout device
    sums holding `samples` samples per pixel, or tile_samples[tile] with a table: colour sums, and unless 0 the sums of
    squares and the albedo, normal and depth sums of render_features_device -> mean radiance, 3 floats per pixel, at
    d_out.  d_scratch: denoise_scratch_bytes(w, h) bytes, 16-byte aligned."""
    v = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    _check(lib().rtw_denoise_device(device, v(d_sum_ptr), v(d_sq_ptr), v(d_albedo_ptr), v(d_normal_ptr),
                                    v(d_depth_ptr), w, h, samples, v(d_tile_samples_ptr), iterations, sigma_l, sigma_n,
                                    sigma_z, v(d_out_ptr), v(d_scratch_ptr), C.c_void_p(stream_ptr)))


def denoise(sums, samples: int, sq=None, albedo=None, normal=None, depth=None, tile_samples=None,
            iterations: int = DENOISE_ITERATIONS, sigma_l: float = DENOISE_SIGMA_L, sigma_n: float = DENOISE_SIGMA_N,
            sigma_z: float = DENOISE_SIGMA_Z) -> np.ndarray:
    """rtw_denoise: denoise_device's arithmetic on the host, no GPU.  sums[h, w, 3] and the optional sq[h, w, 3],
    albedo[h, w, 3], normal[h, w, 3], depth[h, w, 2] hold `samples` samples per pixel, or tile_samples[tile] with a
    table (then `samples` may be 0) -> mean radiance[h, w, 3]."""
    s = np.ascontiguousarray(sums, np.float32)
    h, w = s.shape[:2]
    opt = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (sq, albedo, normal, depth)]
    for a, ch, name in zip(opt, (3, 3, 3, 2), ("sq", "albedo", "normal", "depth")):
        if a is not None and a.shape != (h, w, ch):
            raise ValueError(f"{name} has shape {a.shape}, the {w}x{h} frame wants {(h, w, ch)}")
    ts = None if tile_samples is None else _ua(tile_samples)
    if ts is not None and ts.size != n_tiles(w, h):
        raise ValueError(f"tile_samples has {ts.size} entries, the {w}x{h} image {n_tiles(w, h)} tiles")
    out = np.empty((h, w, 3), np.float32)
    _check(lib().rtw_denoise(_fp(s), *[None if a is None else _fp(a) for a in opt], w, h, samples,
                             None if ts is None else _up(ts), iterations, sigma_l, sigma_n, sigma_z, _fp(out)))
    return out


_FRAME_KEYS = ("sum", "sq", "albedo", "normal", "depth")  # an accumulated frame's buffers before its count
_FRAME_CH = {"sum": 3, "sq": 3, "albedo": 3, "normal": 3, "depth": 2, "count": 1}


def temporal_device(cur: dict, w: int, h: int, samples: int, cam: "Camera", out: dict, hist=None, hist_cam=None,
                    max_history=None, tol_z: float = TEMPORAL_TOL_Z, cos_n: float = TEMPORAL_COS_N,
                    d_tile_samples_ptr: int = 0, device: int = -1, stream_ptr: int = 0):
    """rtw_temporal_device: enqueue temporal accumulation (include/rtw.h defines it).  cur, hist and out map "sum", "sq",
    "albedo", "normal", "depth" (hist and out: and "count") to device addresses of full-layout buffers; a missing key or
    0 is NULL.  The current frame holds `samples` samples per pixel (or tile_samples[tile]) and was rendered with `cam`;
    hist (or None: no history) is an accumulated frame rendered with hist_cam, reprojected onto cam and added with at
    most max_history effective samples (None: TEMPORAL_MAX_HISTORY_FRAMES * samples).  An out buffer may be its
    current-frame buffer, never a history buffer."""
    v = lambda d, k: C.c_void_p(d[k]) if d and d.get(k) else None  # noqa: E731
    if max_history is None:
        max_history = float(TEMPORAL_MAX_HISTORY_FRAMES * samples)
    _check(lib().rtw_temporal_device(
        device, *[v(cur, k) for k in _FRAME_KEYS], w, h, samples, C.c_void_p(d_tile_samples_ptr) if d_tile_samples_ptr
        else None, C.byref(cam.c), *[v(hist, k) for k in _FRAME_KEYS + ("count",)],
        C.byref(hist_cam.c) if hist_cam is not None else None, max_history, tol_z, cos_n,
        *[v(out, k) for k in _FRAME_KEYS + ("count",)], C.c_void_p(stream_ptr)))


def temporal(cur: dict, samples: int, cam: "Camera", hist=None, hist_cam=None, max_history=None,
             tol_z: float = TEMPORAL_TOL_Z, cos_n: float = TEMPORAL_COS_N, tile_samples=None, in_place: bool = False):
    """rtw_temporal: temporal_device's arithmetic on the host, no GPU.  cur maps "sum"[h, w, 3], "depth"[h, w, 2] and
    optionally "sq", "albedo", "normal"[h, w, 3] to the current frame's sums (a key missing or None: NULL); hist (or
    None) is an accumulated frame with the same keys and "count"[h, w].  -> the accumulated frame, a dict of the keys
    in use and "count"; in_place writes each output over its current-frame array (C-contiguous float32) and returns
    those."""
    if in_place:
        c = {k: a for k, a in cur.items() if a is not None}
        if any(a.dtype != np.float32 or not a.flags.c_contiguous or not a.flags.writeable for a in c.values()):
            raise ValueError("in_place wants writable C-contiguous float32 arrays")
    else:
        c = {k: np.ascontiguousarray(a, np.float32) for k, a in cur.items() if a is not None}
    h, w = c["sum"].shape[:2]
    hs = None if hist is None else {k: np.ascontiguousarray(a, np.float32) for k, a in hist.items() if a is not None}
    for d, keys in ((c, _FRAME_KEYS), (hs or {}, _FRAME_KEYS + ("count",))):
        for k, a in d.items():
            want = (h, w) if k == "count" else (h, w, _FRAME_CH[k])
            if k not in keys or a.shape != want:
                raise ValueError(f"{k} has shape {a.shape}, the {w}x{h} frame wants {want}")
    ts = None if tile_samples is None else _ua(tile_samples)
    if ts is not None and ts.size != n_tiles(w, h):
        raise ValueError(f"tile_samples has {ts.size} entries, the {w}x{h} image {n_tiles(w, h)} tiles")
    out = {k: (a if in_place else np.empty_like(a)) for k, a in c.items()}
    out["count"] = np.empty((h, w), np.float32)
    if max_history is None:
        max_history = float(TEMPORAL_MAX_HISTORY_FRAMES * samples)
    p = lambda d, k: _fp(d[k]) if d and k in d else None  # noqa: E731
    _check(lib().rtw_temporal(
        *[p(c, k) for k in _FRAME_KEYS], w, h, samples, None if ts is None else _up(ts), C.byref(cam.c),
        *[p(hs, k) for k in _FRAME_KEYS + ("count",)], C.byref(hist_cam.c) if hist_cam is not None else None,
        max_history, tol_z, cos_n, *[p(out, k) for k in _FRAME_KEYS + ("count",)]))
    return out


def denoise_counts_device(d_sum_ptr: int, d_sq_ptr: int, d_albedo_ptr: int, d_normal_ptr: int, d_depth_ptr: int,
                          d_count_ptr: int, w: int, h: int, d_out_ptr: int, d_scratch_ptr: int,
                          iterations: int = DENOISE_ITERATIONS, sigma_l: float = DENOISE_SIGMA_L,
                          sigma_n: float = DENOISE_SIGMA_N, sigma_z: float = DENOISE_SIGMA_Z, device: int = -1,
                          stream_ptr: int = 0):
    """rtw_denoise_counts_device: denoise_device for an accumulated frame, whose sample count is d_count's float per
    pixel (temporal_device's out "count"); a pixel is empty unless its count is > 0.  Scratch as denoise_device's."""
    v = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    _check(lib().rtw_denoise_counts_device(device, v(d_sum_ptr), v(d_sq_ptr), v(d_albedo_ptr), v(d_normal_ptr),
                                           v(d_depth_ptr), v(d_count_ptr), w, h, iterations, sigma_l, sigma_n, sigma_z,
                                           v(d_out_ptr), v(d_scratch_ptr), C.c_void_p(stream_ptr)))


def denoise_counts(sums, count, sq=None, albedo=None, normal=None, depth=None, iterations: int = DENOISE_ITERATIONS,
                   sigma_l: float = DENOISE_SIGMA_L, sigma_n: float = DENOISE_SIGMA_N,
                   sigma_z: float = DENOISE_SIGMA_Z) -> np.ndarray:
    """rtw_denoise_counts: denoise_counts_device's arithmetic on the host, no GPU.  count[h, w] holds each pixel's
    sample count -> mean radiance[h, w, 3]."""
    s = np.ascontiguousarray(sums, np.float32)
    h, w = s.shape[:2]
    cnt = np.ascontiguousarray(count, np.float32)
    if cnt.shape != (h, w):
        raise ValueError(f"count has shape {cnt.shape}, the {w}x{h} frame wants {(h, w)}")
    opt = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (sq, albedo, normal, depth)]
    for a, ch, name in zip(opt, (3, 3, 3, 2), ("sq", "albedo", "normal", "depth")):
        if a is not None and a.shape != (h, w, ch):
            raise ValueError(f"{name} has shape {a.shape}, the {w}x{h} frame wants {(h, w, ch)}")
    out = np.empty((h, w, 3), np.float32)
    _check(lib().rtw_denoise_counts(_fp(s), *[None if a is None else _fp(a) for a in opt], _fp(cnt), w, h, iterations,
                                    sigma_l, sigma_n, sigma_z, _fp(out)))
    return out


class TemporalRenderer:
    """A sequence of few-sample frames over one committed scene, each accumulated onto the reprojected history of the
    frames before it and denoised, all on the device.  frame(cam) renders frame k = 0, 1, ... with seed + k: the
    generator is keyed by (seed, j, i, sample), so one seed for every frame would repeat each pixel's noise from frame
    to frame -- screen-locked noise, correlated with the history it is averaged with, which would then be worthless.
    Per frame: render_samples_device with the squares plus render_features_device into one of two device buffer sets
    (torch tensors on cuda:device), temporal_device in place against the other set, then denoise_counts_device.
    reset() drops the history: the next frame stands alone (its seed still advances)."""

    def __init__(self, scene: Scene, background, image_width: int, image_height: int, samples_per_pixel: int,
                 seed: int = 0, max_depth: int = 50, device: int = 0):
        self.scene, self.bg = scene, _fa(background)
        self.w, self.h, self.spp = int(image_width), int(image_height), int(samples_per_pixel)
        self.seed, self.max_depth, self.device = int(seed), int(max_depth), int(device)
        self.k = 0
        self._hist_cam = None
        self._bufs = None

    def reset(self) -> None:
        self._hist_cam = None

    def _ptrs(self, t) -> dict:
        px, b = self.w * self.h, t.data_ptr()
        return {k: b + 4 * px * o for k, o in zip(_FRAME_KEYS + ("count",), (0, 3, 6, 9, 12, 14))}

    def frame(self, cam: Camera, denoise: bool = True, max_history=None, tol_z: float = TEMPORAL_TOL_Z,
              cos_n: float = TEMPORAL_COS_N, iterations: int = DENOISE_ITERATIONS, sigma_l: float = DENOISE_SIGMA_L,
              sigma_n: float = DENOISE_SIGMA_N, sigma_z: float = DENOISE_SIGMA_Z):
        """-> (mean radiance[h, w, 3] in render()'s row order, stats of the colour samples with "frame": k,
        "history": whether one was used, and "count": the accumulated frame's effective samples[h, w]).  denoise=False
        returns the accumulated frame's own mean, sum / count (+0 where the count is 0)."""
        import torch

        px, dev = self.w * self.h, self.device
        if self._bufs is None:
            td = torch.device("cuda", dev)
            self._bufs = ([torch.empty(px * 15, dtype=torch.float32, device=td) for _ in range(2)],
                          torch.empty(denoise_scratch_bytes(self.w, self.h), dtype=torch.uint8, device=td),
                          torch.empty(px * 3, dtype=torch.float32, device=td))
        sets, scratch, out = self._bufs
        cur_t, hist_t = sets[self.k & 1], sets[(self.k & 1) ^ 1]
        cur, hist = self._ptrs(cur_t), self._ptrs(hist_t)
        cur_t.zero_()
        torch.cuda.synchronize(dev)
        rt = Raytracer(self.scene, cam, self.bg, self.w, self.h, self.spp, seed=self.seed + self.k,
                       max_depth=self.max_depth)
        st = rt.render_samples_device(cur["sum"], cur["sq"], device=dev, want_stats=True)
        rt.render_features_device(cur["albedo"], cur["normal"], cur["depth"], device=dev)
        used = self._hist_cam is not None
        temporal_device(cur, self.w, self.h, self.spp, cam, cur, hist if used else None, self._hist_cam,
                        max_history=max_history, tol_z=tol_z, cos_n=cos_n, device=dev)
        if denoise:
            denoise_counts_device(*[cur[k] for k in _FRAME_KEYS + ("count",)], self.w, self.h, out.data_ptr(),
                                  scratch.data_ptr(), iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n,
                                  sigma_z=sigma_z, device=dev)
        torch.cuda.synchronize(dev)
        acc = cur_t.cpu().numpy()
        count = acc[14 * px:].reshape(self.h, self.w)
        if denoise:
            mean = out.cpu().numpy().reshape(self.h, self.w, 3)
        else:
            with np.errstate(all="ignore"):
                mean = np.where(count[..., None] > 0, acc[:3 * px].reshape(self.h, self.w, 3) / count[..., None],
                                np.float32(0.0)).astype(np.float32)
        st.update(frame=self.k, history=used, count=count.copy())
        self._hist_cam = Camera(rtw_camera.from_buffer_copy(cam.c))
        self.k += 1
        return mean, st



def tile_noise_device(d_sum_ptr: int, d_sq_ptr: int, w: int, h: int, samples: int, threshold: float, d_err_ptr: int,
                      d_ids_out_ptr: int, d_n_out_ptr: int, d_ids_in_ptr: int = 0, n_in=None,
                      d_tile_samples_ptr: int = 0, device: int = -1, stream_ptr: int = 0):
    """rtw_tile_noise_device: enqueue the per-tile noise estimate of full-layout device sums holding `samples` samples
    per pixel; d_ids_in_ptr = 0 tests every tile.  err (and tile_samples, unless 0) by global tile id; the ids of the
    tiles above the threshold, in input order, to d_ids_out (room for n_in ids) and their number to d_n_out."""
    n = n_tiles(w, h) if n_in is None else n_in
    _check(lib().rtw_tile_noise_device(device, C.c_void_p(d_sum_ptr), C.c_void_p(d_sq_ptr), w, h,
                                       C.c_void_p(d_ids_in_ptr) if d_ids_in_ptr else None, n, samples, threshold,
                                       C.c_void_p(d_err_ptr), C.c_void_p(d_tile_samples_ptr) if d_tile_samples_ptr else None,
                                       C.c_void_p(d_ids_out_ptr), C.c_void_p(d_n_out_ptr), C.c_void_p(stream_ptr)))


def tonemap_tiles(sums: np.ndarray, tile_samples) -> np.ndarray:
    """rtw_tonemap_tiles: tonemap() of sums[h, w, 3] with a sample count per 8x8 tile (0 = black) -> uint8[h, w, 3]."""
    s = np.ascontiguousarray(sums, np.float32)
    h, w = s.shape[:2]
    ts = _ua(tile_samples)
    if ts.size != n_tiles(w, h):
        raise ValueError(f"tile_samples has {ts.size} entries, the {w}x{h} image {n_tiles(w, h)} tiles")
    out = np.empty(s.shape, np.uint8)
    _check(lib().rtw_tonemap_tiles(_fp(s.reshape(-1)), w, h, _up(ts), out.ctypes.data_as(_U8)))
    return out


def tonemap_tiles_device(d_sum_ptr: int, w: int, h: int, d_tile_samples_ptr: int, d_rgb8_ptr: int, device: int = -1,
                         stream_ptr: int = 0):
    """tonemap_tiles() over device arrays, enqueued on a stream."""
    _check(lib().rtw_tonemap_tiles_device(device, C.c_void_p(d_sum_ptr), w, h, C.c_void_p(d_tile_samples_ptr),
                                          C.c_void_p(d_rgb8_ptr), C.c_void_p(stream_ptr)))


def sample_blocks(sample_first: int, n_samples: int) -> list:
    """rtw_sample_blocks -> [(first, log2 of the size)]: the aligned power-of-two blocks, in order, that
    render_samples_device runs the range as (host only)."""
    first, log2 = np.zeros(62, np.uint32), np.zeros(62, np.uint32)
    n = C.c_uint32()
    _check(lib().rtw_sample_blocks(sample_first, n_samples, _up(first), _up(log2), 62, C.byref(n)))
    return [(int(first[k]), int(log2[k])) for k in range(n.value)]


def tonemap_device(d_sum_ptr: int, n_pixels: int, spp: int, d_rgb8_ptr: int, device: int = -1, stream_ptr: int = 0):
    """tonemap() over device arrays (n_pixels x 3 float sums -> n_pixels x 3 bytes), enqueued on a stream."""
    _check(lib().rtw_tonemap_device(device, C.c_void_p(d_sum_ptr), n_pixels, spp, C.c_void_p(d_rgb8_ptr),
                                    C.c_void_p(stream_ptr)))


def make_rays(origins, directions, times=None, streams=None) -> np.ndarray:
    """rtw_ray records (RAY_DTYPE) from [n, 3] origins and directions, times [n] and stream words [n]."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    rays = np.zeros(len(o), RAY_DTYPE)
    rays["origin"] = o
    rays["direction"] = np.asarray(directions, np.float32).reshape(-1, 3)
    if times is not None:
        rays["time"] = np.asarray(times, np.float32).reshape(-1)
    if streams is not None:
        rays["stream"] = np.asarray(streams, np.uint64).reshape(-1)
    return rays


def progress_encode(kind: int, width=0, height=0, spp=0, pixel=None) -> bytes:
    """postcard::to_vec_cobs(&ProgressMessage) (lib.rs:128-138): COBS frame incl. its 0x00."""
    m = rtw_progress_msg(kind=kind, width=width, height=height, samples_per_pixel=spp)
    if pixel is not None:
        m.pixel.row, m.pixel.column = int(pixel[0]), int(pixel[1])
        m.pixel.color[:] = [float(x) for x in pixel[2]]
    out = (C.c_uint8 * 64)()
    n = C.c_size_t()
    _check(lib().rtw_progress_encode(C.byref(m), out, 64, C.byref(n)))
    return bytes(out[:n.value])


def progress_decode(frame: bytes) -> dict:
    """postcard::from_bytes_cobs::<ProgressMessage> (discovery_host_receiver/src/main.rs:37)."""
    buf = (C.c_uint8 * max(1, len(frame))).from_buffer_copy(frame or b"\0")
    m = rtw_progress_msg()
    _check(lib().rtw_progress_decode(buf, len(frame), C.byref(m)))
    d = {"kind": int(m.kind)}
    if m.kind == MSG_IMAGE_START:
        d.update(width=int(m.width), height=int(m.height), samples_per_pixel=int(m.samples_per_pixel))
    elif m.kind == MSG_PIXEL:
        d.update(row=int(m.pixel.row), column=int(m.pixel.column), color=[float(x) for x in m.pixel.color])
    return d


def perlin_generate(seed: int = 0):
    """Perlin::new(rng) (perlin.rs:14-48) with the build's seeded stream -> (grad[256, 3], perm[3, 256])."""
    g = np.zeros(768, np.float32)
    p = np.zeros(768, np.uint32)
    _check(lib().rtw_perlin_generate(seed, _fp(g), _up(p)))
    return g.reshape(256, 3), p.reshape(3, 256)


def preset_cameras(name: str, aspect: float, models_dir=None) -> list:
    """Every camera of a preset (scenes.rs World's Vec<Camera>): 30 for animated-book2-final-scene."""
    n = C.c_uint32()
    md = str(models_dir or MODELS_DIR).encode()
    _check(lib().rtw_preset_cameras(name.encode(), aspect, md, None, 0, C.byref(n)))
    cams = (rtw_camera * max(1, n.value))()
    _check(lib().rtw_preset_cameras(name.encode(), aspect, md, cams, n.value, C.byref(n)))
    return [Camera(cams[k]) for k in range(n.value)]


def unpack_tiles_device(w, h, d_tiles_ptr, n_tiles, d_packed_ptr, d_image_ptr, device=-1, stream_ptr=0):
    _check(lib().rtw_unpack_tiles_device(device, w, h, C.c_void_p(d_tiles_ptr), n_tiles, C.c_void_p(d_packed_ptr),
                                         C.c_void_p(d_image_ptr), C.c_void_p(stream_ptr)))


def diag_libm(fn: int, a, b=None) -> np.ndarray:
    """Device f32 transcendentals (0 log10f, 1 sinf, 2 acosf, 3 atan2f(a, b)) and the camera's
    division (4: a / b by Markstein's correction from RN(1 / b)) and the sphere test's sqrt (5) over
    host arrays."""
    a = _fa(a)
    bb = _fa(b) if b is not None else None
    out = np.empty_like(a)
    _check(lib().rtw_diag_libm(fn, len(a), _fp(a), _fp(bb) if bb is not None else None, _fp(out)))
    return out


def diag_sweep(fn: int, lo: int = 0, hi: int = 0xFFFFFFFF, cap: int = 64):
    """Device fast path vs the IEEE operation over every bit pattern in [lo, hi] (fn 0: reciprocal)
    -> (mismatches, skipped, first mismatching patterns)."""
    counts = (C.c_uint64 * 2)()
    bad = np.zeros(max(1, cap), np.uint32)
    _check(lib().rtw_diag_sweep(fn, lo, hi, counts, _up(bad), cap))
    return int(counts[0]), int(counts[1]), bad[:min(cap, int(counts[0]))]


def diag_recip(b) -> np.ndarray:
    """The host's RN(1 / b) behind the camera divisions (no device needed)."""
    b = _fa(b)
    out = np.empty_like(b)
    _check(lib().rtw_diag_recip(len(b), _fp(b), _fp(out)))
    return out


def diag_tile_beam(cam, w: int, h: int, tile: int, box_lo, box_hi) -> bool:
    """The tile lists' beam test for one tile and one box (host only): may a camera ray of the tile meet the box?"""
    lo, hi = _fa(box_lo), _fa(box_hi)
    rc = lib().rtw_diag_tile_beam(C.byref(cam.c), w, h, tile, _fp(lo), _fp(hi))
    if rc < 0:
        _check(rc)
    return bool(rc)


def diag_tile_lists(scene, cam, w: int, h: int, device: int = 0):
    """rtw_diag_tile_lists -> (per tile a list of BVH primitive indices, or None for a tile on overflow; the overflow
    count; the DFS key of every BVH primitive, by index)."""
    nt = n_tiles(w, h)
    rec = np.zeros(nt * 8, np.uint32)
    over = C.c_uint32()
    keys = np.zeros(65536, np.uint32)
    n = lib().rtw_diag_tile_lists(scene._p, device, C.byref(cam.c), w, h, _up(rec), rec.size, C.byref(over),
                                  _up(keys), keys.size)
    if n < 0:
        _check(n)
    half = rec.view(np.uint16).reshape(nt, 16)
    lists = [None if r[0] == 0xFFFF else [int(x) for x in r[1:1 + int(r[0])]] for r in half]
    return lists, int(over.value), keys[:n]


def tile_partition(w: int, h: int, n_parts: int, part: int):
    """rtw_tile_partition -> (padded ids of the part [ceil(nt / n_parts)], number of real ids)."""
    nt = n_tiles(w, h)
    per = (nt + n_parts - 1) // n_parts if n_parts > 0 else 0
    ids = np.zeros(max(1, per), np.uint32)
    n = C.c_uint32()
    _check(lib().rtw_tile_partition(w, h, n_parts, part, _up(ids), per, C.byref(n)))
    return ids[:per], int(n.value)


def n_tiles(w: int, h: int) -> int:
    return ((w + 7) // 8) * ((h + 7) // 8)


def tonemap(sums: np.ndarray, spp: int) -> np.ndarray:
    """console_app/src/main.rs:68-90 -> uint8 image of the same shape."""
    s = np.ascontiguousarray(sums, np.float32)
    out = np.empty(s.shape, np.uint8)
    _check(lib().rtw_tonemap(_fp(s.reshape(-1)), s.size // 3, spp, out.ctypes.data_as(_U8)))
    return out


def image_height(width: int, aspect: float = 1.7777778) -> int:
    """console_app/src/main.rs:33: (width as f64 / aspect).round() as u32 (ties away from zero)."""
    import math
    x = width / aspect
    return int(math.floor(x + 0.5))


def camera_aspect(width: int, height: int) -> float:
    """console_app/src/main.rs:39: (w as f32) / (h as f32)."""
    return float(np.float32(width) / np.float32(height))
