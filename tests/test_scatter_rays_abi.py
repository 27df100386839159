"""rtw_scatter_rays* / rtw_camera_rays* (Material::scatter + emitted, Camera::get_ray) without a GPU: rtw_scatter's
layout in the header, the ctypes mirror, the numpy dtype, INTEGRATION.md's Rust block and the compiled header, and the
argument checks of all four calls.

As for rtw_hit_rays (tests/test_hit_rays_abi.py) the checks come in the render calls' order -- a NULL argument, the
scene's state, the host scans (a zero stream word; the frame, the path range and the shutter), then the device copy --
so each is reachable on a machine without a GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_integration_abi import ROOT, ctypes_fields, header, integration_rust, rust_funcs, rust_structs

FUNCS = ("rtw_camera_rays", "rtw_camera_rays_device", "rtw_scatter_rays", "rtw_scatter_rays_device")
BG = (0.7, 0.8, 1.0)
W, H, SPP = 13, 7, 3


def test_fields_match_header_ctypes_numpy_and_rust(rtw):
    structs, _, _ = header()
    want = structs["rtw_scatter"]
    assert want == [("attenuation", "[f32;3]"), ("emitted", "[f32;3]"), ("flags", "u32"), ("reserved", "u32")]
    assert ctypes_fields(rtw.rtw_scatter) == want, "ctypes rtw_scatter differs from include/rtw.h"
    assert rust_structs(integration_rust())["RtwScatter"] == want, "RtwScatter differs from include/rtw.h"
    dt, st = rtw.SCATTER_DTYPE, rtw.rtw_scatter
    assert dt.itemsize == C.sizeof(st) == 32
    assert [(f, dt.fields[f][1]) for f, _t in st._fields_] == [(f, getattr(st, f).offset) for f, _t in st._fields_]
    assert [dt.fields[f][1] for f, _t in st._fields_] == [0, 12, 24, 28]
    rust = integration_rust()
    for name, value in (("SCATTERED", 1), ("MISS", 2), ("BAD", 4)):
        assert getattr(rtw, f"SCATTER_{name}") == value
        assert f"pub const RTW_SCATTER_{name}: u32 = {value};" in rust


def test_size_and_flags_match_compiled_header(rtw, tmp_path):
    structs, _, _ = header()
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT / "include" / "rtw.h"}"', "int main(void){",
             'printf("rtw_scatter %zu\\n", sizeof(rtw_scatter));']
    for f, _t in structs["rtw_scatter"]:
        lines.append(f'printf("rtw_scatter.{f} %zu\\n", offsetof(rtw_scatter, {f}));')
    lines.append('printf("flags %d %d %d\\n", RTW_SCATTER_SCATTERED, RTW_SCATTER_MISS, RTW_SCATTER_BAD);')
    lines.append('printf("abi %d\\n", RTW_ABI_VERSION);')
    lines.append("return 0;}")
    prog, exe = tmp_path / "sz.c", tmp_path / "sz"
    prog.write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(ln.split(None, 1) for ln in out if ln)
    assert int(got["rtw_scatter"]) == C.sizeof(rtw.rtw_scatter) == 32
    for f, _t in rtw.rtw_scatter._fields_:
        assert int(got[f"rtw_scatter.{f}"]) == getattr(rtw.rtw_scatter, f).offset, f
    assert got["flags"].split() == ["1", "2", "4"]
    assert got["abi"] == "7", "the new calls are additive: the ABI version stays"


def test_functions_are_declared_everywhere(rtw):
    _, funcs, _ = header()
    rf = rust_funcs(integration_rust())
    for name in FUNCS:
        assert name in funcs and name in rf and name in rtw.EXPORTED_SYMBOLS, name
        assert hasattr(rtw.lib(), name), name
        assert len(rtw._SIGS[name][1]) == len(funcs[name][1]), name
    assert funcs["rtw_scatter_rays"][1] == ["p(m)RtwScene", "i32", "u64", "p(c)c_void", "p(c)c_void", "p(c)f32",
                                            "p(m)c_void", "p(m)c_void", "p(m)RtwStats"]
    assert funcs["rtw_camera_rays"][1] == ["p(m)RtwScene", "i32", "p(c)RtwCamera", "u32", "u32", "u32", "u64", "u64",
                                           "u64", "p(m)c_void", "p(m)RtwStats"]


# ---------------------------------------------------------------- argument checks
def _world(rtw):
    """Moving spheres committed over [0, 1], on whatever devices there are: (scene, there is a device copy)."""
    s = rtw.Scene()
    m = s.lambertian_solid((0.5, 0.5, 0.5))
    s.sphere((0, 0, -3), 1.0, m)
    s.moving_sphere((2, 0, -3), 0.0, (2, 0.5, -3), 1.0, 0.5, m)
    if rtw.device_count() > 0:
        s.commit()
        return s, True
    with pytest.raises(rtw.RtwError) as e:
        s.commit()
    assert e.value.code == rtw.RTW_ENODEV
    return s, False


def _camera(rtw, t0=0.0, t1=1.0):
    return rtw.Camera.new((0, 0, 2), (0, 0, -3), (0, 1, 0), 40.0, W / H, 0.1, 5.0, t0, t1)


def _records(rtw, n=5):
    """n rays towards the first sphere with non-zero stream words, and hit records for them (front-face hits of
    material 0 at z = -2)."""
    rays = rtw.make_rays(np.zeros((n, 3)), np.tile([0.0, 0.0, -1.0], (n, 1)), np.full(n, 0.5), np.arange(1, n + 1))
    hits = np.zeros(n, rtw.HIT_DTYPE)
    hits["p"], hits["normal"], hits["t"] = (0, 0, -2), (0, 0, 1), 2.0
    hits["flags"] = rtw.HIT_HIT | rtw.HIT_FRONT_FACE
    return rays, hits


def _scatter(rtw, s, rays, hits, device_call, n=None, null=()):
    """rtw_scatter_rays[_device] with the arguments named in `null` passed as NULL -> its return code."""
    L = rtw.lib()
    n = len(rays) if n is None else n
    out, sc = np.zeros(max(1, len(rays)), rtw.RAY_DTYPE), np.zeros(max(1, len(rays)), rtw.SCATTER_DTYPE)
    bg = np.asarray(BG, np.float32)
    a = {"rays": rays.ctypes.data if len(rays) else None, "hits": hits.ctypes.data if len(hits) else None,
         "bg": bg.ctypes.data_as(C.POINTER(C.c_float)), "out": out.ctypes.data, "sc": sc.ctypes.data}
    for k in null:
        a[k] = None
    sp = None if "scene" in null else s._p
    if device_call:
        return L.rtw_scatter_rays_device(sp, 0, n, a["rays"], a["hits"], a["bg"], a["out"], a["sc"], None, None)
    cast = lambda p, t: C.cast(C.c_void_p(p), C.POINTER(t))  # noqa: E731
    return L.rtw_scatter_rays(sp, -1, n, cast(a["rays"], rtw.rtw_ray), cast(a["hits"], rtw.rtw_hit), a["bg"],
                              cast(a["out"], rtw.rtw_ray), cast(a["sc"], rtw.rtw_scatter), None)


def _camera_call(rtw, s, cam, device_call, w=W, h=H, spp=SPP, first=0, n=None, null=()):
    L = rtw.lib()
    n = w * h * spp - first if n is None else n
    rays = np.zeros(max(1, min(n, 1 << 16)), rtw.RAY_DTYPE)
    rp = None if "rays" in null else rays.ctypes.data
    cp = None if "cam" in null else C.byref(cam.c)
    sp = None if "scene" in null else s._p
    if device_call:
        return L.rtw_camera_rays_device(sp, 0, cp, w, h, spp, 11, first, n, rp, None, None)
    return L.rtw_camera_rays(sp, -1, cp, w, h, spp, 11, first, n, C.cast(C.c_void_p(rp), C.POINTER(rtw.rtw_ray)), None)


@pytest.mark.parametrize("device_call", [False, True])
@pytest.mark.parametrize("null", ["scene", "rays", "hits", "bg", "out", "sc"])
def test_scatter_null_arguments(rtw, device_call, null):
    s, _ = _world(rtw)
    rays, hits = _records(rtw)
    assert _scatter(rtw, s, rays, hits, device_call, null=(null,)) == rtw.RTW_EINVAL
    assert "NULL" in rtw.lib().rtw_last_error().decode()
    # a NULL argument is reported before the scene's state, as by the render calls
    if null != "scene":
        assert _scatter(rtw, rtw.Scene(), rays, hits, device_call, null=(null,)) == rtw.RTW_EINVAL


@pytest.mark.parametrize("device_call", [False, True])
@pytest.mark.parametrize("null", ["scene", "cam", "rays"])
def test_camera_null_arguments(rtw, device_call, null):
    s, _ = _world(rtw)
    assert _camera_call(rtw, s, _camera(rtw), device_call, null=(null,)) == rtw.RTW_EINVAL
    assert "NULL" in rtw.lib().rtw_last_error().decode()
    if null != "scene":
        assert _camera_call(rtw, rtw.Scene(), _camera(rtw), device_call, null=(null,)) == rtw.RTW_EINVAL


@pytest.mark.parametrize("device_call", [False, True])
def test_uncommitted_scene(rtw, device_call):
    s = rtw.Scene()
    s.sphere((0, 0, -3), 1.0, s.lambertian_solid((0.5, 0.5, 0.5)))
    rays, hits = _records(rtw)
    assert _scatter(rtw, s, rays, hits, device_call) == rtw.RTW_ESTATE
    assert "not committed" in rtw.lib().rtw_last_error().decode()
    assert _camera_call(rtw, s, _camera(rtw), device_call) == rtw.RTW_ESTATE
    assert "not committed" in rtw.lib().rtw_last_error().decode()


@pytest.mark.parametrize("device_call", [False, True])
def test_nothing_to_do_is_ok(rtw, device_call):
    s, _ = _world(rtw)
    rays, hits = _records(rtw, 0)
    assert _scatter(rtw, s, rays, hits, device_call) == 0
    assert _scatter(rtw, s, rays, hits, device_call, null=("rays", "hits", "out", "sc")) == 0  # no array is looked at
    assert _camera_call(rtw, s, _camera(rtw), device_call, n=0) == 0
    assert _camera_call(rtw, s, _camera(rtw), device_call, n=0, null=("rays",)) == 0
    assert _camera_call(rtw, s, _camera(rtw), device_call, first=W * H * SPP, n=0) == 0  # the empty range at the end


def test_zero_stream_word_is_einval_from_the_host_call(rtw):
    """xoroshiro64* never leaves state 0 and the materials' rejection loops are unbounded: the host call scans the
    stream words before anything is enqueued, so this needs no device."""
    s, _ = _world(rtw)
    rays, hits = _records(rtw)
    rays["stream"][3] = 0
    assert _scatter(rtw, s, rays, hits, False) == rtw.RTW_EINVAL
    msg = rtw.lib().rtw_last_error().decode()
    assert "record 3" in msg and "stream" in msg
    with pytest.raises(rtw.RtwError) as e:
        s.scatter_rays(rays, hits, BG)
    assert e.value.code == rtw.RTW_EINVAL


@pytest.mark.parametrize("device_call", [False, True])
def test_camera_frame_range_and_shutter_are_checked_on_the_host(rtw, device_call):
    s, _ = _world(rtw)
    L = rtw.lib()
    assert _camera_call(rtw, s, _camera(rtw, 0.0, 2.0), device_call) == rtw.RTW_EINVAL  # committed over [0, 1]
    assert "shutter" in L.rtw_last_error().decode()
    assert _camera_call(rtw, s, _camera(rtw), device_call, w=65537, n=4) == rtw.RTW_EINVAL
    assert "65536" in L.rtw_last_error().decode()
    assert _camera_call(rtw, s, _camera(rtw), device_call, h=65537, n=4) == rtw.RTW_EINVAL
    assert _camera_call(rtw, s, _camera(rtw), device_call, first=0, n=W * H * SPP + 1) == rtw.RTW_EINVAL
    assert "leave the frame" in L.rtw_last_error().decode()
    assert _camera_call(rtw, s, _camera(rtw), device_call, first=100, n=W * H * SPP - 99) == rtw.RTW_EINVAL
    assert _camera_call(rtw, s, _camera(rtw), device_call, first=2 ** 64 - 1, n=2) == rtw.RTW_EINVAL  # no wrap-around
    assert _camera_call(rtw, s, _camera(rtw), device_call, w=1, n=1) == rtw.RTW_EINVAL  # lib.rs:84 divides by w - 1


@pytest.mark.parametrize("which", ["d_rays", "d_hits", "d_out_rays", "d_out_scatter", "camera d_rays"])
def test_device_forms_want_16_byte_aligned_arrays(rtw, which):
    """Checked on the host before the device copy is looked for, so with or without a GPU; and not at all for n = 0,
    which looks at no array."""
    s, _ = _world(rtw)
    L = rtw.lib()
    buf = np.zeros(4 * 48 + 16, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    bg = np.asarray(BG, np.float32).ctypes.data_as(C.POINTER(C.c_float))

    def call(n):
        if which == "camera d_rays":
            return L.rtw_camera_rays_device(s._p, 0, C.byref(_camera(rtw).c), W, H, SPP, 11, 0, n, C.c_void_p(base + 8),
                                            None, None)
        p = {k: base + (8 if k == which else 0) for k in ("d_rays", "d_hits", "d_out_rays", "d_out_scatter")}
        return L.rtw_scatter_rays_device(s._p, 0, n, p["d_rays"], p["d_hits"], bg, p["d_out_rays"], p["d_out_scatter"],
                                         None, None)

    assert call(3) == rtw.RTW_EINVAL
    assert "16-byte aligned" in L.rtw_last_error().decode()
    assert call(0) == 0


def test_without_a_device_copy(rtw):
    """A scene that rtw_scene_commit flattened: RTW_ENODEV where there is no GPU (never a CPU fallback), the records
    where there is one."""
    s, on_device = _world(rtw)
    rays, hits = _records(rtw)
    cam = _camera(rtw)
    if not on_device:
        assert _scatter(rtw, s, rays, hits, False) == rtw.RTW_ENODEV
        assert _scatter(rtw, s, rays, hits, True) in (rtw.RTW_ENODEV, rtw.RTW_EINVAL)  # (host pointers)
        assert _camera_call(rtw, s, cam, False) == rtw.RTW_ENODEV
        assert _camera_call(rtw, s, cam, True) in (rtw.RTW_ENODEV, rtw.RTW_EINVAL)
        for call in (lambda: s.scatter_rays(rays, hits, BG), lambda: s.camera_rays(cam, W, H, SPP, 11)):
            with pytest.raises(rtw.RtwError) as e:
                call()
            assert e.value.code == rtw.RTW_ENODEV
    else:
        out, sc = s.scatter_rays(rays, hits, BG)
        assert (sc["flags"] == rtw.SCATTER_SCATTERED).all() and (sc["attenuation"] == np.float32(0.5)).all()
        assert (out["origin"] == hits["p"]).all() and (out["time"] == rays["time"]).all()
        assert len(s.camera_rays(cam, W, H, SPP, 11)) == W * H * SPP
