"""ctypes binding of the CPU oracle (oracle/_build/liboracle.so).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg, always as the checker / the timed CPU baseline, never by the product.
See rtw_oracle.c's header for what it restates and its parity status.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

ORACLE_DIR = Path(__file__).resolve().parent
LIB_PATH = ORACLE_DIR / "_build" / "liboracle.so"

ITERATIVE, RECURSIVE = 0, 1
BVH_AS_LIST, BVH_REFERENCE = 0, 1


class oracle_camera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("lower_left_corner", C.c_float * 3),
                ("horizontal", C.c_float * 3), ("vertical", C.c_float * 3),
                ("u", C.c_float * 3), ("v", C.c_float * 3), ("w", C.c_float * 3),
                ("lens_radius", C.c_float), ("time0", C.c_float), ("time1", C.c_float)]


_F = C.POINTER(C.c_float)
_U32 = C.POINTER(C.c_uint32)
_U64 = C.POINTER(C.c_uint64)
_lib = None

# The records of the caller-ray entries (rtw_oracle.h: oracle_hit, oracle_scattered, oracle_sample).  Fields are named
# as the product's HIT_DTYPE, SCATTER_DTYPE + RAY_DTYPE and SAMPLE_DTYPE name them, and the flag values are the product's.
HIT_HIT, HIT_FRONT_FACE = 1, 2
SCATTER_SCATTERED, SCATTER_MISS = 1, 2
END_MISS, END_NO_SCATTER, END_DEPTH = 1, 2, 8
HIT_RECORD = np.dtype([("p", np.float32, 3), ("normal", np.float32, 3), ("t", np.float32), ("u", np.float32),
                       ("v", np.float32), ("material", np.uint32), ("flags", np.uint32)])
SCATTER_RECORD = np.dtype([("attenuation", np.float32, 3), ("emitted", np.float32, 3), ("origin", np.float32, 3),
                           ("direction", np.float32, 3), ("time", np.float32), ("flags", np.uint32),
                           ("stream", np.uint64)])
SAMPLE_RECORD = np.dtype([("color", np.float32, 3), ("segments", np.uint32), ("stream", np.uint64),
                          ("flags", np.uint32), ("reserved", np.uint32)])
assert (HIT_RECORD.itemsize, SCATTER_RECORD.itemsize, SAMPLE_RECORD.itemsize) == (44, 64, 32)


def build() -> None:
    subprocess.run(["make", "-s", "-C", str(ORACLE_DIR)], check=True)


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            build()
        L = C.CDLL(str(LIB_PATH))
        sig = {
            "oracle_scene_parse": (C.c_void_p, [C.c_char_p, C.POINTER(C.c_void_p), C.c_int]),
            "oracle_scene_free": (None, [C.c_void_p]),
            "oracle_last_error": (C.c_char_p, []),
            "oracle_scene_count": (C.c_int, [C.c_void_p, C.c_int]),
            "oracle_camera_new": (None, [_F, _F, _F, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                         C.c_float, C.POINTER(oracle_camera)]),
            "oracle_render": (C.c_int, [C.c_void_p, C.POINTER(oracle_camera), _F, C.c_uint32, C.c_uint32,
                                        C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_int, _U32,
                                        C.c_uint32, _F, C.POINTER(C.c_uint64)]),
            "oracle_render_counts": (C.c_int, [C.c_void_p, C.POINTER(oracle_camera), _F, C.c_uint32, C.c_uint32,
                                               C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_int, _U32,
                                               C.c_uint32, _F, C.POINTER(C.c_uint64), _U32]),
            "oracle_render_pixels": (C.c_int, [C.c_void_p, C.POINTER(oracle_camera), _F, C.c_uint32, C.c_uint32,
                                               C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_int, _U32,
                                               C.c_uint32, _F, C.POINTER(C.c_uint64)]),
            "oracle_pcg32_stream": (C.c_uint32, [C.c_uint64, C.c_uint32, _U32, C.POINTER(C.c_uint64)]),
            "oracle_rng_stream": (C.c_uint32, [C.c_uint64, C.c_uint32, _U32, C.POINTER(C.c_uint64)]),
            "oracle_splitmix64": (C.c_uint64, [C.c_uint64]),
            "oracle_path_state": (C.c_uint64, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]),
            "oracle_u32_to_f32": (C.c_float, [C.c_uint32]),
            "oracle_u32_to_range": (C.c_float, [C.c_uint32, C.c_float, C.c_float]),
            "oracle_u64_to_f64": (C.c_double, [C.c_uint64]),
            "oracle_sphere_uv": (None, [_F, _F]),
            "oracle_hit_primitive": (C.c_int, [C.c_int, _F, _F, C.c_float, C.c_float, _F]),
            "oracle_aabb_hit": (C.c_int, [_F, _F, _F, C.c_float, C.c_float]),
            "oracle_scatter": (C.c_int, [C.c_int, _F, _F, _F, _U32, C.c_uint32, _F, _U32]),
            "oracle_get_ray": (None, [C.POINTER(oracle_camera), C.c_float, C.c_float, _U32, C.c_uint32, _F,
                                      _U32]),
            "oracle_tonemap": (C.c_uint8, [C.c_float, C.c_uint32]),
            "oracle_libm": (C.c_int, [C.c_int, C.c_uint32, _F, _F, _F]),
            "oracle_medium_hit": (C.c_int, [C.c_int, _F, C.c_float, _F, C.c_float, C.c_float, C.c_uint64,
                                            C.c_uint32, _F]),
            "oracle_noise": (C.c_float, [_F, C.POINTER(C.c_int32), _F, C.c_int]),
            "oracle_hit_rays": (C.c_int, [C.c_void_p, C.c_uint64, _F, _U64, C.c_int, C.c_void_p, C.c_void_p]),
            "oracle_scatter_rays": (C.c_int, [C.c_void_p, C.c_uint64, _F, _U64, C.c_void_p, _F, C.c_void_p]),
            "oracle_sample_rays": (C.c_int, [C.c_void_p, C.c_uint64, _F, _U64, _F, C.c_uint32, C.c_int, C.c_int,
                                             C.c_void_p]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def f32(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1))


def fp(a: np.ndarray):
    return a.ctypes.data_as(_F)


def camera_new(look_from, look_at, vup, vfov, aspect, aperture, focus, t0=0.0, t1=1.0) -> oracle_camera:
    c = oracle_camera()
    lib().oracle_camera_new(fp(f32(look_from)), fp(f32(look_at)), fp(f32(vup)), vfov, aspect, aperture,
                            focus, t0, t1, C.byref(c))
    return c


def camera_from_fields(d: dict) -> oracle_camera:
    c = oracle_camera()
    for k, _ in oracle_camera._fields_:
        v = d[k]
        if isinstance(v, (list, tuple)):
            getattr(c, k)[:] = [float(x) for x in v]
        else:
            setattr(c, k, float(v))
    return c


class OracleScene:
    """A scene parsed from rtw_scene_dump() text (+ image texture buffers)."""

    def __init__(self, text: str, images=()):
        self._imgs = [np.ascontiguousarray(i, np.uint8) for i in images]
        arr = (C.c_void_p * max(1, len(self._imgs)))(*[i.ctypes.data for i in self._imgs])
        self._p = lib().oracle_scene_parse(text.encode(), arr, len(self._imgs))
        if not self._p:
            raise RuntimeError(lib().oracle_last_error().decode())

    def __del__(self):
        if getattr(self, "_p", None) and _lib is not None:  # (None at interpreter exit, where module-level caches
            _lib.oracle_scene_free(self._p)                 # of scenes are collected after this module's globals)
            self._p = None

    def count(self, what: int) -> int:
        return lib().oracle_scene_count(self._p, what)

    def render(self, cam: oracle_camera, background, w, h, spp, seed=0, max_depth=50,
               integrator=ITERATIVE, bvh_mode=BVH_AS_LIST, threads=None, rows=None, pixel_rays=False):
        """-> (sums[h, w, 3] in reference order, rays[, per-pixel rays[h, w] when pixel_rays]).
        rows: list of j (bottom-based) to render."""
        out = np.zeros((h, w, 3), np.float32)
        rays = C.c_uint64()
        pr = np.zeros((h, w), np.uint32) if pixel_rays else None
        r = np.ascontiguousarray(rows, np.uint32) if rows is not None else None
        n = threads or min(16, os.cpu_count() or 1)  # the GPU box's CPU share is 16
        rc = lib().oracle_render_counts(self._p, C.byref(cam), fp(f32(background)), w, h, spp, max_depth, seed,
                                        integrator, bvh_mode, n, r.ctypes.data_as(_U32) if r is not None else None,
                                        len(r) if r is not None else 0, fp(out), C.byref(rays),
                                        pr.ctypes.data_as(_U32) if pr is not None else None)
        if rc != 0:
            raise RuntimeError(lib().oracle_last_error().decode())
        return (out, int(rays.value), pr) if pixel_rays else (out, int(rays.value))

    def render_pixels(self, cam: oracle_camera, background, w, h, spp, pixels, seed=0, max_depth=50,
                      integrator=ITERATIVE, bvh_mode=BVH_AS_LIST, threads=None):
        """-> (sums[n, 3], rays) of the given (j, i) pixels (j bottom-based), in their order."""
        px = np.ascontiguousarray(np.asarray(pixels, np.uint32).reshape(-1, 2))
        out = np.zeros((len(px), 3), np.float32)
        rays = C.c_uint64()
        n = threads or min(16, os.cpu_count() or 1)
        rc = lib().oracle_render_pixels(self._p, C.byref(cam), fp(f32(background)), w, h, spp, max_depth, seed,
                                        integrator, bvh_mode, n, px.ctypes.data_as(_U32), len(px), fp(out),
                                        C.byref(rays))
        if rc != 0:
            raise RuntimeError(lib().oracle_last_error().decode())
        return out, int(rays.value)

    # ---- rays the caller chooses (records with origin, direction, time and stream fields, as the product's RAY_DTYPE)
    @staticmethod
    def _rays(rays):
        r7 = np.ascontiguousarray(np.concatenate([rays["origin"], rays["direction"], rays["time"][:, None]], axis=1),
                                  np.float32)
        return r7, np.ascontiguousarray(rays["stream"], np.uint64)

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(lib().oracle_last_error().decode())

    def hit_rays(self, rays, bvh_mode=BVH_AS_LIST, ties=False):
        """world.hit(ray, 0.001, inf) per ray -> HIT_RECORD records (material: the index in the dump's table)[, a bool
        per ray: two or more objects hit at the winner's t exactly]."""
        r7, st = self._rays(rays)
        out = np.zeros(len(r7), HIT_RECORD)
        tie = np.zeros(len(r7), np.uint8)
        self._check(lib().oracle_hit_rays(self._p, len(r7), fp(r7), st.ctypes.data_as(_U64), bvh_mode, out.ctypes.data,
                                          tie.ctypes.data if ties else None))
        return (out, tie != 0) if ties else out

    def scatter_rays(self, rays, hits, background) -> np.ndarray:
        """Material::emitted + scatter for (ray, hit record) pairs -> SCATTER_RECORD records.  hits: records with
        HIT_RECORD's fields (the product's HIT_DTYPE has them)."""
        r7, st = self._rays(rays)
        h = np.zeros(len(r7), HIT_RECORD)
        for name in HIT_RECORD.names:
            h[name] = hits[name]
        out = np.zeros(len(r7), SCATTER_RECORD)
        self._check(lib().oracle_scatter_rays(self._p, len(r7), fp(r7), st.ctypes.data_as(_U64), h.ctypes.data,
                                              fp(f32(background)), out.ctypes.data))
        return out

    def sample_rays(self, rays, background, max_depth=50, integrator=ITERATIVE, bvh_mode=BVH_AS_LIST) -> np.ndarray:
        """sample_ray per ray -> SAMPLE_RECORD records (the product's SAMPLE_DTYPE, field for field)."""
        r7, st = self._rays(rays)
        out = np.zeros(len(r7), SAMPLE_RECORD)
        self._check(lib().oracle_sample_rays(self._p, len(r7), fp(r7), st.ctypes.data_as(_U64), fp(f32(background)),
                                             max_depth, integrator, bvh_mode, out.ctypes.data))
        return out


def libm(fn: int, a, b=None) -> np.ndarray:
    """The oracle's f32 transcendentals (0 log10f, 1 sinf, 2 acosf, 3 atan2f(a, b))."""
    a = f32(a)
    bb = f32(b) if b is not None else None
    out = np.empty_like(a)
    if lib().oracle_libm(fn, len(a), fp(a), fp(bb) if bb is not None else None, fp(out)) != 0:
        raise ValueError(fn)
    return out


def noise(grad, perm, p, depth: int = 7) -> float:
    """perlin.rs noise (depth 0) / turbulence(p, depth) over explicit tables."""
    g = f32(grad)
    pm = np.ascontiguousarray(np.asarray(perm, np.int32).reshape(-1))
    return float(lib().oracle_noise(fp(g), pm.ctypes.data_as(C.POINTER(C.c_int32)), fp(f32(p)), depth))
