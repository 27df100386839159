#!/usr/bin/env python3
"""What the adaptive loop costs and what it buys: python scripts/adaptive_cost.py [--parent-lib PATH]

jumpy-balls 1920x1080, min_spp 16, max_spp 512 on one MI355X.  Every run is a process of its own (one warm-up, one timed
run), so that two libraries never share one; each prints the kernel time (HIP events, summed over the calls or rounds),
the wall time of the whole sequence between two device synchronisations, and the rays.
  ranges    rtw_render_samples_device over [0,16) [16,32) [32,64) [64,128) [128,256) [256,512), all tiles, with the sums
            of squares: what the adaptive call does at threshold 0 without its noise test.  Of --parent-lib (a
            librtw_amd.so built from the parent commit, bound by hand) when given, else of this build;
  adaptive  rtw_render_adaptive_device at a threshold, with the histogram of tile_samples;
  one_shot  rtw_render_device at 512 spp.
Overhead: `ranges` and `adaptive 0` alternated, five runs each, medians compared.  Then adaptive at three thresholds and
the one-shot frame.  Nothing asserts a time; the ray counts of `ranges`, `adaptive 0` and `one_shot` must agree when no
tile stops early at threshold 0.
"""
import ctypes as C
import importlib.util
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
W, H, MIN_SPP, MAX_SPP, MAX_DEPTH, SEED, SCENE_SEED = 1920, 1080, 16, 512, 50, 7, 42
RANGES = [(0, 16), (16, 16), (32, 32), (64, 64), (128, 128), (256, 256)]
THRESHOLDS = (0.05, 0.02, 0.01)
WARMUP, PAIRS, LIMIT_S = 1, 5, 300


def load_rtw():
    pkg = ROOT / "raytracer-weekend_amd"
    spec = importlib.util.spec_from_file_location("rtw_amd", pkg / "__init__.py", submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["rtw_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def ranges_of(lib_path):
    """the six ranges through the library at lib_path, bound by hand (an older library lacks the newer symbols)"""
    import torch
    rtw = load_rtw()
    L = C.CDLL(str(lib_path))
    for name in ("rtw_scene_create", "rtw_scene_preset", "rtw_scene_commit", "rtw_render_samples_device"):
        getattr(L, name).restype, getattr(L, name).argtypes = rtw._SIGS[name]
    p, cam, bg = C.c_void_p(), rtw.rtw_camera(), np.zeros(3, np.float32)
    fp = bg.ctypes.data_as(C.POINTER(C.c_float))
    assert L.rtw_scene_create(C.byref(p)) == 0
    assert L.rtw_scene_preset(p, b"jumpy-balls", W / H, SCENE_SEED, str(rtw.MODELS_DIR).encode(), C.byref(cam), fp) == 0
    assert L.rtw_scene_commit(p, 0) == 0
    d_sum = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0")
    d_sq = torch.zeros_like(d_sum)
    out = {}
    for _ in range(WARMUP + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d_sum.zero_()
        d_sq.zero_()
        ms, rays = 0.0, 0
        for first, n in RANGES:
            st = rtw.rtw_stats()
            assert L.rtw_render_samples_device(p, 0, C.byref(cam), fp, W, H, first, n, MAX_DEPTH, SEED, None, 0,
                                               C.c_void_p(d_sum.data_ptr()), C.c_void_p(d_sq.data_ptr()), None, 0,
                                               C.byref(st)) == 0
            ms += float(st.kernel_ms)
            rays += int(st.rays)
        torch.cuda.synchronize()
        out = {"kernel_ms": round(ms, 3), "wall_ms": round((time.perf_counter() - t0) * 1e3, 3), "rays": rays}
    print(json.dumps(out))


def adaptive(threshold):
    import torch
    rtw = load_rtw()
    s = rtw.Scene()
    cam, bg = s.preset("jumpy-balls", W / H, seed=SCENE_SEED)
    s.commit(device=0)
    rt = rtw.Raytracer(s, cam, bg, W, H, MAX_SPP, seed=SEED, max_depth=MAX_DEPTH)
    nt = rtw.n_tiles(W, H)
    d_sum = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0")
    d_sq = torch.zeros_like(d_sum)
    d_ts = torch.zeros(nt, dtype=torch.int32, device="cuda:0")
    d_err = torch.zeros(nt, dtype=torch.float32, device="cuda:0")
    out = {}
    for _ in range(WARMUP + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = rt.render_adaptive_device(threshold, d_sum.data_ptr(), d_sq.data_ptr(), d_ts.data_ptr(), d_err.data_ptr(),
                                       min_spp=MIN_SPP, device=0, want_stats=True)
        torch.cuda.synchronize()
        ts = d_ts.cpu().numpy()
        out = {"threshold": threshold, "kernel_ms": round(st["kernel_ms"], 3),
               "wall_ms": round((time.perf_counter() - t0) * 1e3, 3), "rays": st["rays"], "paths": st["paths"],
               "tile_samples": {int(n): int((ts == n).sum()) for n in np.unique(ts)}, "lib_sha": rtw.lib_sha()}
    print(json.dumps(out))


def one_shot():
    import torch
    rtw = load_rtw()
    s = rtw.Scene()
    cam, bg = s.preset("jumpy-balls", W / H, seed=SCENE_SEED)
    s.commit(device=0)
    rt = rtw.Raytracer(s, cam, bg, W, H, MAX_SPP, seed=SEED, max_depth=MAX_DEPTH)
    d_img = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0")
    st = [rt.render_device(d_img.data_ptr(), 0, want_stats=True) for _ in range(WARMUP + 1)][-1]
    print(json.dumps({"kernel_ms": round(st["kernel_ms"], 3), "rays": st["rays"], "paths": st["paths"]}))


def child(*args):
    r = subprocess.run([sys.executable, __file__, *args], timeout=LIMIT_S, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{args}: exit status {r.returncode}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    if sys.argv[1:2] == ["--ranges"]:
        return ranges_of(sys.argv[2])
    if sys.argv[1:2] == ["--adaptive"]:
        return adaptive(float(sys.argv[2]))
    if sys.argv[1:2] == ["--one-shot"]:
        return one_shot()
    own = ROOT / "raytracer-weekend_amd" / "lib" / "librtw_amd.so"
    base = sys.argv[2] if sys.argv[1:2] == ["--parent-lib"] else str(own)
    res = {"ranges_lib": "parent" if base != str(own) else "this build", "ranges": [], "adaptive_0": []}
    for _ in range(PAIRS):
        res["ranges"].append(child("--ranges", base))
        res["adaptive_0"].append(child("--adaptive", "0"))
        print(json.dumps({"ranges": res["ranges"][-1], "adaptive_0": res["adaptive_0"][-1]}), flush=True)
    for k in ("kernel_ms", "wall_ms"):
        a = float(np.median([x[k] for x in res["adaptive_0"]]))
        b = float(np.median([x[k] for x in res["ranges"]]))
        res[f"ratio_{k}"] = round(a / b, 4)
    res["thresholds"] = [child("--adaptive", repr(t)) for t in THRESHOLDS]
    res["one_shot"] = child("--one-shot")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
