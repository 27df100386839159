"""rtw_hit_rays / rtw_hit_rays_device (Hittable::hit, hittable/mod.rs:22-69) without a GPU: the two records'
layout in the header, the ctypes mirror and INTEGRATION.md's Rust block, and the argument checks of the host call.

The argument checks come in the render calls' order -- a NULL argument, the scene's state, then the rays' times, then
the device copy -- so every one of them is reachable on a machine without a GPU: rtw_scene_commit flattens the scene
before it looks for a device, and a scene that got that far answers RTW_ENODEV, not RTW_ESTATE."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_integration_abi import ROOT, ctypes_fields, header, integration_rust, rust_structs

STRUCTS = {"rtw_ray": "RtwRay", "rtw_hit": "RtwHit"}


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_fields_match_header_ctypes_and_rust(rtw, cname):
    structs, _, _ = header()
    want = structs[cname]
    assert ctypes_fields(getattr(rtw, cname)) == want, f"ctypes {cname} differs from include/rtw.h"
    assert rust_structs(integration_rust())[STRUCTS[cname]] == want, f"{STRUCTS[cname]} differs from include/rtw.h"
    dt = {"rtw_ray": rtw.RAY_DTYPE, "rtw_hit": rtw.HIT_DTYPE}[cname]
    st = getattr(rtw, cname)
    assert dt.itemsize == C.sizeof(st)
    assert [(f, dt.fields[f][1]) for f, _t in st._fields_] == [(f, getattr(st, f).offset) for f, _t in st._fields_]


def test_sizes_match_compiled_header(rtw, tmp_path):
    """sizeof / offsetof of rtw_ray and rtw_hit as the C compiler lays the header out == the ctypes mirror's (the
    Rust #[repr(C)] layout follows the same C rules from the same field list, compared above)."""
    structs, _, _ = header()
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT / "include" / "rtw.h"}"', "int main(void){"]
    for cname in STRUCTS:
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _t in structs[cname]:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('printf("flags %d %d %d\\n", RTW_HIT_HIT, RTW_HIT_FRONT_FACE, RTW_HIT_BAD_RAY);')
    lines.append("return 0;}")
    prog, exe = tmp_path / "sz.c", tmp_path / "sz"
    prog.write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(ln.split(None, 1) for ln in out if ln)
    assert (int(got["rtw_ray"]), int(got["rtw_hit"])) == (40, 48)
    for cname in STRUCTS:
        st = getattr(rtw, cname)
        assert int(got[cname]) == C.sizeof(st), cname
        for f, _t in st._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(st, f).offset, (cname, f)
    assert got["flags"].split() == [str(rtw.HIT_HIT), str(rtw.HIT_FRONT_FACE), str(rtw.HIT_BAD_RAY)] == ["1", "2", "4"]


def test_abi_version_is_7(rtw):
    assert rtw.lib().rtw_abi_version() == rtw.ABI_VERSION == 7


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


def _call(rtw, s, rays, hits=True, n=None, device_call=False):
    L = rtw.lib()
    n = len(rays) if n is None else n
    out = np.zeros(max(1, len(rays)), rtw.HIT_DTYPE)
    rp = rays.ctypes.data_as(C.POINTER(rtw.rtw_ray)) if len(rays) else None
    hp = out.ctypes.data_as(C.POINTER(rtw.rtw_hit)) if hits else None
    if device_call:
        return L.rtw_hit_rays_device(s._p if s else None, 0, n, C.cast(rp, C.c_void_p), C.cast(hp, C.c_void_p), None,
                                     None), out
    return L.rtw_hit_rays(s._p if s else None, -1, n, rp, hp, None), out


def _rays(rtw, n=3, time=0.5):
    return rtw.make_rays(np.zeros((n, 3)), np.tile([0.0, 0.0, -1.0], (n, 1)), np.full(n, time))


@pytest.mark.parametrize("device_call", [False, True])
def test_null_arguments(rtw, device_call):
    s, _ = _world(rtw)
    rays = _rays(rtw)
    assert _call(rtw, None, rays, device_call=device_call)[0] == rtw.RTW_EINVAL
    assert _call(rtw, s, rays, hits=False, device_call=device_call)[0] == rtw.RTW_EINVAL
    assert _call(rtw, s, rays[:0], n=3, device_call=device_call)[0] == rtw.RTW_EINVAL  # NULL rays, n > 0
    # a NULL argument is reported before the scene's state, as by the render calls
    assert _call(rtw, rtw.Scene(), rays, hits=False, device_call=device_call)[0] == rtw.RTW_EINVAL


@pytest.mark.parametrize("device_call", [False, True])
def test_uncommitted_scene(rtw, device_call):
    s = rtw.Scene()
    s.sphere((0, 0, -3), 1.0, s.lambertian_solid((0.5, 0.5, 0.5)))
    assert _call(rtw, s, _rays(rtw), device_call=device_call)[0] == rtw.RTW_ESTATE
    assert "not committed" in rtw.lib().rtw_last_error().decode()


@pytest.mark.parametrize("device_call", [False, True])
def test_no_rays_is_ok(rtw, device_call):
    s, _ = _world(rtw)
    assert _call(rtw, s, _rays(rtw, 0), device_call=device_call)[0] == 0
    assert _call(rtw, s, _rays(rtw, 0), hits=False, device_call=device_call)[0] == 0  # no array is looked at


@pytest.mark.parametrize("time", [float("nan"), -0.25, 1.5, float("inf")])
def test_bad_time_is_einval_from_the_host_call(rtw, time):
    """The BVH's moving-sphere boxes bound the committed shutter [0, 1] only: the host call scans the times before
    anything is enqueued, so this needs no device."""
    s, _ = _world(rtw)
    rays = _rays(rtw, 5)
    rays["time"][3] = time
    rc, _out = _call(rtw, s, rays)
    assert rc == rtw.RTW_EINVAL
    msg = rtw.lib().rtw_last_error().decode()
    assert "ray 3" in msg and "motion range" in msg


@pytest.mark.parametrize("which", ["d_rays", "d_hits"])
def test_device_form_wants_16_byte_aligned_arrays(rtw, which):
    """Checked on the host before the device copy is looked for, so with or without a GPU; and not at all for n = 0,
    which looks at no array."""
    s, _ = _world(rtw)
    L = rtw.lib()
    buf = np.zeros(4 * 48 + 16, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    ptr = {"d_rays": base, "d_hits": base}
    ptr[which] += 8
    args = (C.c_void_p(ptr["d_rays"]), C.c_void_p(ptr["d_hits"]), None, None)
    assert L.rtw_hit_rays_device(s._p, 0, 3, *args) == rtw.RTW_EINVAL
    assert "16-byte aligned" in L.rtw_last_error().decode()
    assert L.rtw_hit_rays_device(s._p, 0, 0, *args) == 0


def test_without_a_device_copy(rtw):
    """A scene that rtw_scene_commit flattened: RTW_ENODEV where there is no GPU (never a CPU fallback), the records
    where there is one."""
    s, on_device = _world(rtw)
    rays = _rays(rtw)
    rc, out = _call(rtw, s, rays)
    if not on_device:
        assert rc == rtw.RTW_ENODEV
        assert _call(rtw, s, rays, device_call=True)[0] in (rtw.RTW_ENODEV, rtw.RTW_EINVAL)  # (host pointers)
        with pytest.raises(rtw.RtwError) as e:
            s.hit_rays(rays["origin"], rays["direction"], rays["time"])
        assert e.value.code == rtw.RTW_ENODEV
    else:
        assert rc == 0
        assert (out["flags"][:3] & rtw.HIT_HIT).all() and np.all(out["t"][:3] == np.float32(2.0))
