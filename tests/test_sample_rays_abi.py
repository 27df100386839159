"""rtw_sample_rays* (Raytracer::sample_ray, lib.rs:97-117, for rays the caller chooses) without a GPU: rtw_sample's
layout in the header, the ctypes mirror, the numpy dtype, INTEGRATION.md's Rust block and the compiled header, the
flag values, the exports, and the argument checks of both calls.

The checks come in the query calls' order (csrc/rtw_query.cpp) -- a NULL argument, the scene's state, n == 0, the host
scan of the records (the device form: the arrays' alignment), then the device copy -- so each is reachable on a machine
without a GPU, where a call that passes them all ends in RTW_ENODEV."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_integration_abi import ROOT, ctypes_fields, header, integration_rust, rust_funcs, rust_structs

FUNCS = ("rtw_sample_rays", "rtw_sample_rays_device")
FLAGS = (("END_MISS", 1), ("END_NO_SCATTER", 2), ("BAD_RAY", 4), ("END_DEPTH", 8))
BG = (0.7, 0.8, 1.0)


def test_fields_match_header_ctypes_numpy_and_rust(rtw):
    structs, _, _ = header()
    want = structs["rtw_sample"]
    assert want == [("color", "[f32;3]"), ("segments", "u32"), ("stream", "u64"), ("flags", "u32"), ("reserved", "u32")]
    assert ctypes_fields(rtw.rtw_sample) == want, "ctypes rtw_sample differs from include/rtw.h"
    assert rust_structs(integration_rust())["RtwSample"] == want, "RtwSample differs from include/rtw.h"
    dt, st = rtw.SAMPLE_DTYPE, rtw.rtw_sample
    assert dt.itemsize == C.sizeof(st) == 32
    assert [(f, dt.fields[f][1]) for f, _t in st._fields_] == [(f, getattr(st, f).offset) for f, _t in st._fields_]
    assert [dt.fields[f][1] for f, _t in st._fields_] == [0, 12, 16, 24, 28]
    rust = integration_rust()
    for name, value in FLAGS:
        assert getattr(rtw, f"SAMPLE_{name}") == value
        assert f"pub const RTW_SAMPLE_{name}: u32 = {value};" in rust


def test_size_offsets_and_flags_match_compiled_header(rtw, tmp_path):
    structs, _, _ = header()
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT / "include" / "rtw.h"}"', "int main(void){",
             'printf("rtw_sample %zu\\n", sizeof(rtw_sample));']
    for f, _t in structs["rtw_sample"]:
        lines.append(f'printf("rtw_sample.{f} %zu\\n", offsetof(rtw_sample, {f}));')
    lines.append('printf("flags %d %d %d %d\\n", RTW_SAMPLE_END_MISS, RTW_SAMPLE_END_NO_SCATTER, RTW_SAMPLE_BAD_RAY, '
                 'RTW_SAMPLE_END_DEPTH);')
    lines.append('printf("abi %d\\n", RTW_ABI_VERSION);')
    lines.append("return 0;}")
    prog, exe = tmp_path / "sz.c", tmp_path / "sz"
    prog.write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(ln.split(None, 1) for ln in out if ln)
    assert int(got["rtw_sample"]) == C.sizeof(rtw.rtw_sample) == 32
    for f, _t in rtw.rtw_sample._fields_:
        assert int(got[f"rtw_sample.{f}"]) == getattr(rtw.rtw_sample, f).offset, f
    assert got["flags"].split() == [str(v) for _n, v in FLAGS]
    assert got["abi"] == "7", "the new calls are additive: the ABI version stays"


def test_functions_are_declared_and_exported_everywhere(rtw):
    _, funcs, _ = header()
    rf = rust_funcs(integration_rust())
    for name in FUNCS:
        assert name in funcs and name in rf and name in rtw.EXPORTED_SYMBOLS, name
        assert hasattr(rtw.lib(), name), name
        assert len(rtw._SIGS[name][1]) == len(funcs[name][1]), name
    assert funcs["rtw_sample_rays"] == ("i32", ["p(m)RtwScene", "i32", "u64", "p(c)c_void", "p(c)f32", "u32",
                                                "p(m)c_void", "p(m)RtwStats"])
    assert funcs["rtw_sample_rays_device"] == ("i32", ["p(m)RtwScene", "i32", "u64", "p(c)c_void", "p(c)f32", "u32",
                                                       "p(m)c_void", "p(m)c_void", "p(m)RtwStats"])
    assert hasattr(rtw.Scene, "sample_rays") and hasattr(rtw.Scene, "sample_rays_device")


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


def _rays(rtw, n=5):
    """n rays towards the first sphere with times in the motion range and non-zero stream words"""
    return rtw.make_rays(np.zeros((n, 3)), np.tile([0.0, 0.0, -1.0], (n, 1)), np.full(n, 0.5), np.arange(1, n + 1))


def _call(rtw, s, rays, device_call, n=None, null=(), max_depth=5, offset=None):
    """rtw_sample_rays[_device] with the arguments named in `null` passed as NULL -> its return code."""
    L = rtw.lib()
    n = len(rays) if n is None else n
    out = np.zeros(max(1, len(rays)) + 1, rtw.SAMPLE_DTYPE)
    bg = np.asarray(BG, np.float32)
    a = {"rays": rays.ctypes.data if len(rays) else None, "bg": bg.ctypes.data_as(C.POINTER(C.c_float)),
         "samples": out.ctypes.data}
    for k in null:
        a[k] = None
    if offset:
        a[offset] += 8
    sp = None if "scene" in null else s._p
    if device_call:
        return L.rtw_sample_rays_device(sp, 0, n, a["rays"], a["bg"], max_depth, a["samples"], None, None)
    cast = lambda p, t: C.cast(C.c_void_p(p), C.POINTER(t))  # noqa: E731
    return L.rtw_sample_rays(sp, -1, n, cast(a["rays"], rtw.rtw_ray), a["bg"], max_depth,
                             cast(a["samples"], rtw.rtw_sample), None)


@pytest.mark.parametrize("device_call", [False, True])
@pytest.mark.parametrize("null", ["scene", "rays", "bg", "samples"])
def test_null_arguments(rtw, device_call, null):
    s, _ = _world(rtw)
    rays = _rays(rtw)
    assert _call(rtw, s, rays, device_call, null=(null,)) == rtw.RTW_EINVAL
    assert "NULL" in rtw.lib().rtw_last_error().decode()
    # a NULL argument is reported before the scene's state
    if null != "scene":
        assert _call(rtw, rtw.Scene(), rays, device_call, null=(null,)) == rtw.RTW_EINVAL


@pytest.mark.parametrize("device_call", [False, True])
def test_uncommitted_scene(rtw, device_call):
    s = rtw.Scene()
    s.sphere((0, 0, -3), 1.0, s.lambertian_solid((0.5, 0.5, 0.5)))
    rays = _rays(rtw)
    assert _call(rtw, s, rays, device_call) == rtw.RTW_ESTATE
    assert "not committed" in rtw.lib().rtw_last_error().decode()
    # the scene's state is reported before the records are scanned / the alignment is looked at
    rays["stream"][2] = 0
    assert _call(rtw, s, rays, device_call, offset="rays") == rtw.RTW_ESTATE


@pytest.mark.parametrize("device_call", [False, True])
def test_nothing_to_do_is_ok(rtw, device_call):
    s, _ = _world(rtw)
    rays = _rays(rtw, 0)
    assert _call(rtw, s, rays, device_call) == 0
    assert _call(rtw, s, rays, device_call, null=("rays", "samples")) == 0  # no array is looked at
    assert _call(rtw, s, _rays(rtw), device_call, n=0, offset="samples") == 0  # nor its alignment
    assert _call(rtw, s, rays, device_call, null=("bg",)) == rtw.RTW_EINVAL  # (the background is no array)
    st = rtw.rtw_stats()
    st.rays = st.paths = 99
    bg = np.asarray(BG, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    assert rtw.lib().rtw_sample_rays(s._p, -1, 0, None, bg, 5, None, C.byref(st)) == 0
    assert st.rays == 0 and st.paths == 0 and st.kernel_ms == 0


@pytest.mark.parametrize("bad,word", [("time", 2.0), ("time", -0.5), ("time", float("nan")), ("stream", 0)])
def test_the_host_call_scans_times_and_stream_words(rtw, bad, word):
    """A time outside the committed motion range [0, 1] or NaN, or a stream word of 0 (xoroshiro64* never leaves that
    state and the materials' rejection loops are unbounded): RTW_EINVAL naming the record, before any device is looked
    for."""
    s, _ = _world(rtw)
    rays = _rays(rtw)
    rays[bad][3] = word
    assert _call(rtw, s, rays, False) == rtw.RTW_EINVAL
    msg = rtw.lib().rtw_last_error().decode()
    assert "ray 3" in msg and bad in msg, msg
    with pytest.raises(rtw.RtwError) as e:
        s.sample_rays(rays, BG, 5)
    assert e.value.code == rtw.RTW_EINVAL
    # the first bad record is the one named
    rays["stream"][1] = 0
    assert _call(rtw, s, rays, False) == rtw.RTW_EINVAL
    assert "ray 1" in rtw.lib().rtw_last_error().decode()


@pytest.mark.parametrize("which", ["rays", "samples"])
def test_device_form_wants_16_byte_aligned_arrays(rtw, which):
    """Checked on the host before the device copy is looked for, so with or without a GPU; the device form does no scan
    of the records (they are device memory): a zero stream word there is not an error of the call."""
    s, _ = _world(rtw)
    rays = _rays(rtw)
    assert rays.ctypes.data % 16 == 0
    assert _call(rtw, s, rays, True, offset=which) == rtw.RTW_EINVAL
    assert "16-byte aligned" in rtw.lib().rtw_last_error().decode()
    assert _call(rtw, s, rays, True, n=0, offset=which) == 0


def test_without_a_device_copy(rtw):
    """A scene that rtw_scene_commit flattened, every check passed: RTW_ENODEV where there is no GPU (never a CPU
    fallback), the records where there is one."""
    s, on_device = _world(rtw)
    rays = _rays(rtw)
    if not on_device:
        assert _call(rtw, s, rays, False) == rtw.RTW_ENODEV
        assert _call(rtw, s, rays, False, max_depth=0) == rtw.RTW_ENODEV
        assert _call(rtw, s, rays, True) == rtw.RTW_ENODEV
        with pytest.raises(rtw.RtwError) as e:
            s.sample_rays(rays, BG, 5)
        assert e.value.code == rtw.RTW_ENODEV
    else:
        out, st = s.sample_rays(rays, BG, 5, want_stats=True)
        assert len(out) == len(rays) and (out["segments"] >= 1).all() and (out["flags"] != 0).all()
        assert st["rays"] == out["segments"].sum() and st["paths"] == len(rays)
