#!/usr/bin/env python3
"""What a progressive step costs: python scripts/render_samples_cost.py [--parent-lib PATH]

jumpy-balls 1920x1080x512 on one MI355X, every figure a stats.kernel_ms (HIP events around the call's launches), one
warm-up and then the median of 3:
  one_shot      rtw_render_device, the frame in one call (path kernel + reduce_kernel);
  chunks_8x64   the same frame through rtw_render_samples_device in 8 chunks of 64 samples (each one aligned block: one
                more launch pair per chunk and a shorter end-of-pass tail), the calls' kernel_ms summed;
  chunk_1x512   the same in one chunk of 512 (accumulate_kernel in reduce_kernel's place, nothing else differs);
each of the last two with and without the sums of squares.  --parent-lib names a librtw_amd.so built from another commit
(the parent's): its rtw_render_device is timed alike in processes of its own, one before and one after this build's,
and the ratios are taken against the median of both.
The chunked frames must equal the one-shot frame bit for bit with equal ray counts; nothing asserts a time.
"""
import ctypes as C
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
W, H, SPP, MAX_DEPTH, SEED, SCENE_SEED = 1920, 1080, 512, 50, 7, 42
WARMUP, RUNS, LIMIT_S = 1, 3, 300


def load_rtw():
    pkg = ROOT / "raytracer-weekend_amd"
    spec = importlib.util.spec_from_file_location("rtw_amd", pkg / "__init__.py", submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["rtw_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def one_shot_of(lib_path):
    """rtw_render_device of the library at lib_path, bound by hand (an older library lacks the newer symbols)"""
    import torch
    rtw = load_rtw()
    L = C.CDLL(str(lib_path))
    for name in ("rtw_scene_create", "rtw_scene_preset", "rtw_scene_commit", "rtw_render_device"):
        getattr(L, name).restype, getattr(L, name).argtypes = rtw._SIGS[name]
    p, cam, bg = C.c_void_p(), rtw.rtw_camera(), np.zeros(3, np.float32)
    fp = bg.ctypes.data_as(C.POINTER(C.c_float))
    assert L.rtw_scene_create(C.byref(p)) == 0
    assert L.rtw_scene_preset(p, b"jumpy-balls", W / H, SCENE_SEED, str(rtw.MODELS_DIR).encode(), C.byref(cam), fp) == 0
    assert L.rtw_scene_commit(p, 0) == 0
    d_img = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0")
    ms, rays = [], 0
    for _ in range(WARMUP + RUNS):
        st = rtw.rtw_stats()
        assert L.rtw_render_device(p, 0, C.byref(cam), fp, W, H, SPP, MAX_DEPTH, SEED, None, 0,
                                   C.c_void_p(d_img.data_ptr()), None, 0, C.byref(st)) == 0
        ms.append(float(st.kernel_ms))
        rays = int(st.rays)
    print(json.dumps({"one_shot_ms": [round(x, 3) for x in ms[WARMUP:]], "rays": rays}))


def measure():
    import torch
    rtw = load_rtw()
    s = rtw.Scene()
    cam, bg = s.preset("jumpy-balls", W / H, seed=SCENE_SEED)
    s.commit(device=0)
    rt = rtw.Raytracer(s, cam, bg, W, H, SPP, seed=SEED, max_depth=MAX_DEPTH)
    d_img = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0")
    d_sum, d_sq = torch.zeros_like(d_img), torch.zeros_like(d_img)
    res = {"lib_sha": rtw.lib_sha(), "kernel": [s.info(k) for k in range(16, 24)]}
    runs = [rt.render_device(d_img.data_ptr(), 0, want_stats=True) for _ in range(WARMUP + RUNS)][WARMUP:]
    res["one_shot_ms"] = [round(x["kernel_ms"], 3) for x in runs]
    res["rays"] = runs[0]["rays"]
    for tag, chunk in (("chunks_8x64", 64), ("chunk_1x512", 512)):
        for sq in (True, False):
            times = []
            for _ in range(WARMUP + RUNS):
                d_sum.zero_()
                d_sq.zero_()
                torch.cuda.synchronize()
                sts = [rt.render_samples_device(d_sum.data_ptr(), d_sq.data_ptr() if sq else 0, a, chunk, device=0,
                                                want_stats=True) for a in range(0, SPP, chunk)]
                assert sum(x["rays"] for x in sts) == res["rays"]
                assert torch.equal(d_sum.view(torch.int32), d_img.view(torch.int32)), tag
                times.append(sum(x["kernel_ms"] for x in sts))
            res[tag + ("_sq_ms" if sq else "_ms")] = [round(x, 3) for x in times[WARMUP:]]
    print(json.dumps(res))


def child(*args):
    r = subprocess.run([sys.executable, __file__, *args], timeout=LIMIT_S, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{args}: exit status {r.returncode}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    if sys.argv[1:2] == ["--child"]:
        return measure()
    if sys.argv[1:2] == ["--child-lib"]:
        return one_shot_of(sys.argv[2])
    parent = sys.argv[2] if sys.argv[1:2] == ["--parent-lib"] else None
    before = child("--child-lib", parent) if parent else None  # the parent before and after: the order's share
    res = child("--child")
    base, whose = float(np.median(res["one_shot_ms"])), "this build's"
    if parent:
        after = child("--child-lib", parent)
        assert before["rays"] == after["rays"] == res["rays"], (before["rays"], after["rays"], res["rays"])
        res["parent_one_shot_ms"] = before["one_shot_ms"] + after["one_shot_ms"]
        base, whose = float(np.median(res["parent_one_shot_ms"])), "the parent library's"
    res["ratios_to"] = whose + " one_shot"
    for k in ("one_shot_ms", "chunks_8x64_sq_ms", "chunks_8x64_ms", "chunk_1x512_sq_ms", "chunk_1x512_ms"):
        res[k.replace("_ms", "_ratio")] = round(float(np.median(res[k])) / base, 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
