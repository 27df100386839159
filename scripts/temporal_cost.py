#!/usr/bin/env python3
"""Cost of temporal accumulation (rtw_temporal_device) beside a device copy of its least traffic and beside the
denoiser that consumes its output: python scripts/temporal_cost.py [scene ...]

For jumpy-balls at 1920x1080 and 2 samples per pixel it renders two frames with all their buffers (colour sums, squares,
albedo, normal, depth: rtw_render_samples_device, rtw_render_features_device), the second from a camera moved sideways
by one pixel of parallax at the focus plane and with the next seed, makes the first an accumulated frame (a call
without history), then times by device events on the stream the calls run on, 3 warm-ups and then 15 launches each:
  (a) rtw_temporal_device, all triples, the defaults, out of place (so that every launch sees the same inputs);
  (b) a device-to-device copy of 116 bytes per pixel: what the pass must move at least once, the current frame's
      56 bytes in and the accumulated frame's 60 bytes out (the taps, up to 4 x 60 bytes per pixel, are reused
      between neighbouring pixels and are not in this floor);
  (c) rtw_denoise_counts_device on (a)'s output, 5 iterations, the defaults.
The child is a process of its own under a time limit, and a failure ends the run.  It prints the medians, the min..max
of the launches, the GB/s that 116 bytes per pixel make of (a) and (b), the share of pixels that took history and the
ratios (a)/(b) and (a)/(c); nothing asserts a time.
"""
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
W, H, SPP, SEED, ITER = 1920, 1080, 2, 7, 5
SCENES = ("jumpy-balls",)
WARMUP, LAUNCHES, LIMIT_S = 3, 15, 500
FLOOR_BYTES = 116
KEYS = (("sum", 3), ("sq", 3), ("albedo", 3), ("normal", 3), ("depth", 2))


def load_rtw(pkg):
    spec = importlib.util.spec_from_file_location("rtw_amd", pkg / "__init__.py", submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["rtw_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def moved(rtw, cam, pixels):
    """the camera moved along its own u by `pixels` pixels of parallax at the focus plane (a pure translation)"""
    c = rtw.rtw_camera.from_buffer_copy(cam.c)
    step = float(np.linalg.norm(list(c.horizontal))) / (W - 1) * pixels
    for k in range(3):
        c.origin[k] += step * c.u[k]
        c.lower_left_corner[k] += step * c.u[k]
    return rtw.Camera(c)


def measure(name, pkg):
    import torch
    rtw = load_rtw(pkg)
    s = rtw.Scene()
    cam0, bg = s.preset(name, W / H, seed=42)
    s.commit(device=0)
    cam1 = moved(rtw, cam0, 1.0)
    dev = "cuda:0"

    def frame():
        d = {k: torch.zeros((H, W, c), dtype=torch.float32, device=dev) for k, c in KEYS}
        d["count"] = torch.zeros((H, W), dtype=torch.float32, device=dev)
        return d

    def ptrs(d):
        return {k: t.data_ptr() for k, t in d.items()}

    hist, cur, out = frame(), frame(), frame()
    torch.cuda.synchronize()
    for d, cam, seed in ((hist, cam0, SEED), (cur, cam1, SEED + 1)):
        rt = rtw.Raytracer(s, cam, bg, W, H, SPP, seed=seed)
        rt.render_samples_device(d["sum"].data_ptr(), d["sq"].data_ptr(), device=0)
        rt.render_features_device(d["albedo"].data_ptr(), d["normal"].data_ptr(), d["depth"].data_ptr(), device=0)
    rtw.temporal_device(ptrs(hist), W, H, SPP, cam0, ptrs(hist), device=0)  # in place, no history: count = SPP
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    scratch = torch.zeros(rtw.denoise_scratch_bytes(W, H), dtype=torch.uint8, device=dev)
    mean = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    src = torch.zeros(W * H * FLOOR_BYTES, dtype=torch.uint8, device=dev)
    dst = torch.zeros_like(src)

    def timed(fn):
        ms = []
        for _ in range(WARMUP + LAUNCHES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(round(e0.elapsed_time(e1), 4))
        return ms[WARMUP:]

    cur_p = {k: v for k, v in ptrs(cur).items() if k != "count"}
    res = {"scene": name, "lib_sha": rtw.lib_sha(), "pixels": W * H, "iterations": ITER}
    res["temporal_ms"] = timed(lambda: rtw.temporal_device(cur_p, W, H, SPP, cam1, ptrs(out), hist=ptrs(hist),
                                                           hist_cam=cam0, device=0, stream_ptr=stream))
    first = {k: t.clone() for k, t in out.items()}
    res["copy_ms"] = timed(lambda: dst.copy_(src))
    o = ptrs(out)
    res["denoise_ms"] = timed(lambda: rtw.denoise_counts_device(*[o[k] for k, _ in KEYS], o["count"], W, H,
                                                                mean.data_ptr(), scratch.data_ptr(), iterations=ITER,
                                                                device=0, stream_ptr=stream))
    rtw.temporal_device(cur_p, W, H, SPP, cam1, ptrs(out), hist=ptrs(hist), hist_cam=cam0, device=0, stream_ptr=stream)
    torch.cuda.synchronize()
    res["repeat_equal"] = all(bool(torch.equal(out[k].view(torch.int32), first[k].view(torch.int32))) for k in out)
    res["took_history"] = float((out["count"] > SPP).float().mean().item())
    res["hit_pixels"] = float((cur["depth"][..., 1] > 0).float().mean().item())
    s.render_status(device=0)
    print(json.dumps(res))


def mm(xs):
    return f"{np.median(xs):.4f} ms ({min(xs):.4f}..{max(xs):.4f})"


def show(res):
    t, c, d = (float(np.median(res[k])) for k in ("temporal_ms", "copy_ms", "denoise_ms"))
    gbs = lambda ms: FLOOR_BYTES * res["pixels"] / (ms * 1e-3) / 1e9  # noqa: E731
    print(f"{res['scene']} {W}x{H}, {SPP} spp; lib {res['lib_sha']}")
    print(f"  (a) rtw_temporal_device {mm(res['temporal_ms'])}: {gbs(t):.0f} GB/s of its {FLOOR_BYTES} B per pixel; "
          f"{res['took_history']:.3f} of the pixels took history ({res['hit_pixels']:.3f} have hits); repeat bit-equal "
          f"{res['repeat_equal']}")
    print(f"  (b) device copy of {FLOOR_BYTES} B per pixel {mm(res['copy_ms'])}: {gbs(c):.0f} GB/s; (a)/(b) {t / c:.2f}")
    print(f"  (c) rtw_denoise_counts_device, {ITER} iterations {mm(res['denoise_ms'])}; (a)/(c) {t / d:.2f}", flush=True)


def main():
    args = sys.argv[1:]
    if len(args) == 2 and args[0] == "--child":
        return measure(args[1], ROOT / "raytracer-weekend_amd")
    for name in args or SCENES:
        r = subprocess.run([sys.executable, __file__, "--child", name], timeout=LIMIT_S, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"{name}: exit status {r.returncode}\n{r.stderr[-2000:]}")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        show(res)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
