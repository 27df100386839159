"""Progressive renders without a GPU (rtw_render_samples_device, rtw_sample_blocks, rtw_render_progressive,
rtw_tonemap_device): the declarations in the header, the ctypes mirror, INTEGRATION.md's Rust and the exports agree;
the compiled header still says ABI 7; rtw_sample_blocks against a restatement of the schedule; and the argument checks
of the calls, which come in the render calls' order -- a NULL argument, the scene's state, the image size, the sample
range, then the device copy -- so each is reachable on a machine without a GPU, where a call that passes them all ends
in RTW_ENODEV.

rtw_render_progressive's prototype writes its sink's type out (include/rtw.h), so the header parser of
test_integration_abi.py, which knows a fixed list of type names, does not list it: it is parsed here, from the header
and from INTEGRATION.md's second Rust block, and held against the rtw_frame_sink typedef."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from test_integration_abi import (ROOT, _strip_c_comments, _strip_rust_comments, c_type, header, integration_rust,
                                  rust_funcs, rust_type)

FUNCS = ("rtw_render_samples_device", "rtw_sample_blocks", "rtw_render_progressive", "rtw_tonemap_device")
SINK = ("i32", ["p(c)f32", "p(c)f32", "u32", "u32", "u32", "p(m)c_void"])
BG = (0.7, 0.8, 1.0)
TWO31 = 1 << 31


# ---------------------------------------------------------------- declarations
def _header_text():
    return _strip_c_comments((ROOT / "include" / "rtw.h").read_text())


def _c_fn_type(ret, params):
    return c_type(ret + " x")[1], [c_type(p)[1] for p in params.split(",")]


def _header_progressive():
    """rtw_render_progressive's prototype -> (return type, parameter types with the sink's as one entry, the sink's)"""
    m = re.search(r"(\w+)\s+rtw_render_progressive\s*\((.*?)\bint\s*\(\*\s*sink\s*\)\s*\(([^)]*)\)\s*,([^)]*)\)\s*;",
                  _header_text(), flags=re.S)
    assert m, "include/rtw.h: rtw_render_progressive with its sink's type written out"
    before = [c_type(p)[1] for p in m.group(2).split(",") if p.strip()]
    after = [c_type(p)[1] for p in m.group(4).split(",") if p.strip()]
    return c_type(m.group(1) + " x")[1], before + ["RtwFrameSink"] + after, _c_fn_type("int", m.group(3))


def _rust_all():
    md = (ROOT / "INTEGRATION.md").read_text()
    return [_strip_rust_comments(b) for b in re.findall(r"```rust\n(.*?)```", md, flags=re.S)]


def test_frame_sink_typedef_matches_prototype_ctypes_and_rust(rtw):
    m = re.search(r"typedef\s+(\w+)\s*\(\*\s*rtw_frame_sink\)\s*\(([^)]*)\)\s*;", _header_text())
    assert m, "include/rtw.h lacks the rtw_frame_sink typedef"
    assert _c_fn_type(m.group(1), m.group(2)) == SINK
    assert _header_progressive()[2] == SINK, "the type written out in rtw_render_progressive is not rtw_frame_sink's"
    r = re.search(r'pub\s+type\s+RtwFrameSink\s*=\s*(?:unsafe\s+)?extern\s+"C"\s+fn\s*\(([^)]*)\)\s*->\s*([^;]+);',
                  integration_rust())
    assert r, "INTEGRATION.md lacks `pub type RtwFrameSink`"
    got = (rust_type(r.group(2)), [rust_type(p.split(":", 1)[1]) for p in r.group(1).split(",") if p.strip()])
    assert got == SINK
    ct = {C.c_int: "i32", C.c_uint32: "u32", C.c_void_p: "p(m)c_void", C.POINTER(C.c_float): "p(c)f32"}
    assert (ct[rtw.FRAME_SINK._restype_], [ct[a] for a in rtw.FRAME_SINK._argtypes_]) == SINK


def test_functions_are_declared_and_exported_everywhere(rtw):
    _, funcs, _ = header()
    rf = rust_funcs(integration_rust())
    for name in FUNCS:
        assert name in rtw.EXPORTED_SYMBOLS and hasattr(rtw.lib(), name), name
    for name in set(FUNCS) - {"rtw_render_progressive"}:
        assert name in funcs and name in rf and funcs[name] == rf[name], name
        assert len(rtw._SIGS[name][1]) == len(funcs[name][1]), name
    assert funcs["rtw_render_samples_device"] == (
        "i32", ["p(m)RtwScene", "i32", "p(c)RtwCamera", "p(c)f32", "u32", "u32", "u32", "u32", "u32", "u64", "p(c)u32",
                "u32", "p(m)f32", "p(m)f32", "p(m)c_void", "u32", "p(m)RtwStats"])
    assert funcs["rtw_sample_blocks"] == ("i32", ["u32", "u32", "p(m)u32", "p(m)u32", "u32", "p(m)u32"])
    assert funcs["rtw_tonemap_device"] == ("i32", ["i32", "p(c)f32", "u32", "u32", "p(m)u8", "p(m)c_void"])
    # rtw_render_progressive: the header's prototype and the Rust declaration (INTEGRATION.md's second block)
    ret, params, _sink = _header_progressive()
    assert (ret, params) == ("i32", ["p(m)RtwScene", "p(c)RtwCamera", "p(c)f32", "u32", "u32", "u32", "u32", "u64",
                                     "u32", "RtwFrameSink", "p(m)c_void", "p(m)RtwStats"])
    decl = [rust_funcs(b) for b in _rust_all()[1:] if "rtw_render_progressive" in b]
    assert len(decl) == 1 and decl[0]["rtw_render_progressive"] == (ret, params)
    sig = rtw._SIGS["rtw_render_progressive"][1]
    assert len(sig) == len(params) and sig[9] is rtw.FRAME_SINK
    for meth in ("render_samples_device", "render_progressive"):
        assert hasattr(rtw.Raytracer, meth), meth
    assert hasattr(rtw, "sample_blocks") and hasattr(rtw, "tonemap_device")


def test_compiled_header_keeps_abi_7_and_the_sink_types_agree(tmp_path):
    """To the C compiler rtw_render_progressive's written-out parameter is an rtw_frame_sink, and the calls are
    additive: RTW_ABI_VERSION stays 7."""
    prog, exe = tmp_path / "abi.c", tmp_path / "abi"
    prog.write_text("\n".join([
        "#include <stdio.h>", f'#include "{ROOT / "include" / "rtw.h"}"',
        "static int sink(const float* a, const float* b, uint32_t w, uint32_t h, uint32_t n, void* u) {",
        "  (void)a; (void)b; (void)w; (void)h; (void)u; return (int)n; }",
        "typedef int (*progressive_fn)(rtw_scene*, const rtw_camera*, const float*, uint32_t, uint32_t, uint32_t,",
        "                              uint32_t, uint64_t, uint32_t, rtw_frame_sink, void*, rtw_stats*);",
        "_Static_assert(__builtin_types_compatible_p(__typeof__(&rtw_render_progressive), progressive_fn),",
        '               "rtw_render_progressive takes an rtw_frame_sink");',
        "int main(void) {",
        "  rtw_frame_sink f = sink;",
        '  printf("abi %d %d\\n", RTW_ABI_VERSION, f(0, 0, 0, 0, 5, 0));',
        "  return 0; }"]))
    subprocess.run(["gcc", "-Wall", "-Wextra", "-Werror", "-o", str(exe), str(prog)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["abi", "7", "5"]


# ---------------------------------------------------------------- the block schedule
def _blocks(first, n):
    """The schedule restated: at each position the largest power of two that divides it (any, at 0) and fits."""
    out, p, end = [], first, first + n
    while p < end:
        size = (p & -p) if p else TWO31
        while size > end - p:
            size //= 2
        out.append((p, size.bit_length() - 1))
        p += size
    return out


def _check_blocks(rtw, first, n):
    got = rtw.sample_blocks(first, n)
    assert got == _blocks(first, n), (first, n)
    assert len(got) <= 62
    p = first
    for k, (b, lg) in enumerate(got):
        size = 1 << lg
        assert b == p and b % size == 0, (first, n, got)  # contiguous, aligned
        # greedy: no aligned power-of-two block twice the size starts here and fits
        assert b % (2 * size) != 0 or b + 2 * size > first + n, (first, n, got)
        for s in {0, 1, size // 2, size - 1} if size > 1 else {0}:
            assert b ^ s == b + s
        p += size
    assert p == first + n
    return got


def test_sample_blocks_edge_cases(rtw):
    assert _check_blocks(rtw, 0, 0) == [] and _check_blocks(rtw, 77, 0) == [] and _check_blocks(rtw, TWO31, 0) == []
    assert _check_blocks(rtw, 0, 1) == [(0, 0)] and _check_blocks(rtw, 5, 1) == [(5, 0)]
    assert _check_blocks(rtw, 0, 13) == [(0, 3), (8, 2), (12, 0)]
    assert _check_blocks(rtw, 0, TWO31) == [(0, 31)]
    assert _check_blocks(rtw, TWO31 - 1, 1) == [(TWO31 - 1, 0)]
    assert [1 << lg for _b, lg in _check_blocks(rtw, 100, 128)] == [4, 8, 16, 64, 32, 4]
    assert len(_check_blocks(rtw, 1, TWO31 - 2)) == 60
    assert len(_check_blocks(rtw, 1, TWO31 - 1)) == 31  # ends at 2^31
    for k in range(31):  # every single aligned block, and every range one short of / one past it
        _check_blocks(rtw, 3 << k if (3 << k) + (1 << k) <= TWO31 else 0, 1 << k)
        _check_blocks(rtw, 1 << k, (1 << k) - 1)
        _check_blocks(rtw, (1 << k) - 1, min((1 << k) + 1, TWO31 - (1 << k) + 1))


def test_sample_blocks_random_ranges(rtw):
    rng = np.random.default_rng(62)
    worst = 0
    for _ in range(4000):
        bits = int(rng.integers(1, 32))
        first = int(rng.integers(0, 1 << bits))
        n = int(rng.integers(0, min(1 << int(rng.integers(1, 32)), TWO31 - first) + 1))
        worst = max(worst, len(_check_blocks(rtw, first, n)))
    assert 1 < worst <= 62


def test_sample_blocks_arguments(rtw):
    L = rtw.lib()
    first, log2, n = (C.c_uint32 * 62)(), (C.c_uint32 * 62)(), C.c_uint32(99)
    assert L.rtw_sample_blocks(100, 128, first, log2, 5, C.byref(n)) == rtw.RTW_EINVAL  # 6 blocks
    assert n.value == 6 and "cap" in L.rtw_last_error().decode()
    assert L.rtw_sample_blocks(100, 128, first, log2, 6, C.byref(n)) == 0 and n.value == 6
    assert L.rtw_sample_blocks(0, 0, None, None, 0, C.byref(n)) == 0 and n.value == 0
    assert L.rtw_sample_blocks(0, 4, first, log2, 62, None) == rtw.RTW_EINVAL
    assert L.rtw_sample_blocks(0, 4, None, log2, 62, C.byref(n)) == rtw.RTW_EINVAL
    assert L.rtw_sample_blocks(0, 4, first, None, 62, C.byref(n)) == rtw.RTW_EINVAL
    for f, m in ((1, TWO31), (TWO31, 1), (0xFFFFFFFF, 0xFFFFFFFF), (0, TWO31 + 1)):
        assert L.rtw_sample_blocks(f, m, first, log2, 62, C.byref(n)) == rtw.RTW_EINVAL, (f, m)
        assert "2^31" in L.rtw_last_error().decode()


# ---------------------------------------------------------------- argument checks
def _world(rtw):
    """One sphere, committed on whatever devices there are: (scene, there is a device copy)."""
    s = rtw.Scene()
    s.sphere((0, 0, -3), 1.0, s.lambertian_solid((0.5, 0.5, 0.5)))
    if rtw.device_count() > 0:
        s.commit()
        return s, True
    with pytest.raises(rtw.RtwError) as e:
        s.commit()
    assert e.value.code == rtw.RTW_ENODEV
    return s, False


def _call(rtw, name, s, null=(), w=16, h=16, first=0, n=4, max_depth=4, calls=None):
    """One of the two render calls with the arguments named in `null` passed as NULL -> its return code.  The device
    pointers are made-up addresses: no call made here on a machine without a GPU gets as far as using them."""
    L = rtw.lib()
    cam = rtw.Camera.new((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 5.0)
    bg = np.asarray(BG, np.float32)
    sp = None if "scene" in null else s._p
    c = None if "cam" in null else C.byref(cam.c)
    b = None if "bg" in null else bg.ctypes.data_as(C.POINTER(C.c_float))
    if name == "rtw_render_samples_device":
        d_sum = None if "out" in null else C.c_void_p(0x1000)
        return L.rtw_render_samples_device(sp, 0, c, b, w, h, first, n, max_depth, 7, None, 0, d_sum, C.c_void_p(0x2000),
                                           None, 0, None)

    def sink(_sum, _sq, _w, _h, done, _user):
        if calls is not None:
            calls.append(done)
        return 0
    cb = rtw.FRAME_SINK() if "out" in null else rtw.FRAME_SINK(sink)
    return L.rtw_render_progressive(sp, c, b, w, h, n, max_depth, 7, first, cb, None, None)


CALLS = ["rtw_render_samples_device", "rtw_render_progressive"]


@pytest.mark.parametrize("null", ["scene", "cam", "bg", "out"])
@pytest.mark.parametrize("name", CALLS)
def test_null_arguments(rtw, name, null):
    """`out` is the device sums, or the sink.  A NULL argument is reported before the scene's state."""
    s, _ = _world(rtw)
    assert _call(rtw, name, s, null=(null,)) == rtw.RTW_EINVAL
    assert "NULL" in rtw.lib().rtw_last_error().decode()
    if null != "scene":
        assert _call(rtw, name, rtw.Scene(), null=(null,)) == rtw.RTW_EINVAL


@pytest.mark.parametrize("name", CALLS)
def test_uncommitted_scene_then_size_then_range(rtw, name):
    fresh = rtw.Scene()
    # the state before the size and the range
    assert _call(rtw, name, fresh) == rtw.RTW_ESTATE
    assert "not committed" in rtw.lib().rtw_last_error().decode()
    assert _call(rtw, name, fresh, w=1, h=1) == rtw.RTW_ESTATE
    assert _call(rtw, name, fresh, n=TWO31 + 1) == rtw.RTW_ESTATE
    s, _ = _world(rtw)
    # a 1x1 image, before the range
    for w, h in ((1, 1), (1, 16), (16, 1)):
        assert _call(rtw, name, s, w=w, h=h) == rtw.RTW_EINVAL
        assert "2x2" in rtw.lib().rtw_last_error().decode()
    assert _call(rtw, name, s, w=1, h=1, n=TWO31 + 1) == rtw.RTW_EINVAL
    assert "2x2" in rtw.lib().rtw_last_error().decode()
    # a range past 2^31, before the device copy
    assert _call(rtw, name, s, n=TWO31 + 1) == rtw.RTW_EINVAL
    assert "2^31" in rtw.lib().rtw_last_error().decode()
    if name == "rtw_render_samples_device":
        for first, n in ((TWO31, 1), (1, TWO31), (0xFFFFFFFF, 0xFFFFFFFF)):
            assert _call(rtw, name, s, first=first, n=n) == rtw.RTW_EINVAL
            assert "2^31" in rtw.lib().rtw_last_error().decode()


@pytest.mark.parametrize("name", CALLS)
def test_without_a_device_copy(rtw, name):
    """Every check passed: RTW_ENODEV where there is no GPU (never a CPU fallback) -- also for a call with nothing to
    do, which the device calls answer after they found their copy -- and no sink call.  Where there is a GPU: the
    steps of a 4-sample frame, and the calls with nothing to do (they touch no buffer)."""
    s, on_device = _world(rtw)
    calls = []
    if on_device:
        if name == "rtw_render_progressive":
            assert _call(rtw, name, s, calls=calls) == 0 and calls == [1, 2, 4]
        else:
            assert _call(rtw, name, s, n=0) == 0 and _call(rtw, name, s, max_depth=0) == 0
        return
    for kw in ({}, {"n": 0}, {"max_depth": 0}, {"first": 5, "n": TWO31 - 5}):
        if name == "rtw_render_progressive" and "first" in kw:
            kw = {"first": 5, "n": TWO31}  # (first is its step)
        assert _call(rtw, name, s, calls=calls, **kw) == rtw.RTW_ENODEV, kw
    assert calls == []
    rt = rtw.Raytracer(s, rtw.Camera.new((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 5.0), BG, 16, 16, 4)
    with pytest.raises(rtw.RtwError) as e:
        if name == "rtw_render_progressive":
            rt.render_progressive(lambda *_a: calls.append(1))
        else:
            rt.render_samples_device(0x1000)
    assert e.value.code == rtw.RTW_ENODEV and calls == []


def test_tonemap_device_arguments(rtw):
    L = rtw.lib()
    assert L.rtw_tonemap_device(-1, None, 4, 1, C.c_void_p(0x1000), None) == rtw.RTW_EINVAL
    assert L.rtw_tonemap_device(-1, C.c_void_p(0x1000), 4, 1, None, None) == rtw.RTW_EINVAL
    assert "NULL" in L.rtw_last_error().decode()
    assert L.rtw_tonemap_device(-1, C.c_void_p(0x1000), 4, 0, C.c_void_p(0x2000), None) == rtw.RTW_EINVAL
    assert "spp" in L.rtw_last_error().decode()
    assert L.rtw_tonemap_device(-1, None, 0, 1, None, None) == 0  # nothing to do
