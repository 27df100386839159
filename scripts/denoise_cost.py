#!/usr/bin/env python3
"""Cost of the denoiser (rtw_denoise_device) beside the same filter in torch tensor ops and beside its traffic floor:
python scripts/denoise_cost.py [scene ...]

For jumpy-balls at 1920x1080 and 4 samples per pixel it renders the colour sums, their squares and the guides once
(rtw_render_samples_device, rtw_render_features_device), then times by device events on the stream the calls run on,
2 warm-ups and then 7 launches each:
  (a) rtw_denoise_device, 5 iterations, the defaults, with the steps' built-in choice of LDS or global taps;
  (b) the same call under RTW_DENOISE_LDS = 0 (every step's taps from global memory), 1 (step 1 through LDS), 2 (step 2),
      3 (both), 4 and 7 (step 4 as well): the LDS decision's numbers.  Steps taken one at a time: 1 iteration with mask
      0 against 1 (prepare + step 1 + finish) and 2 iterations with mask 0 against 2 (the same + step 2);
  (c) the same filter written with torch tensor ops on the GPU (torch_denoise below: one tensor op per f32 operation of
      include/rtw.h's definition, the taps in the contract's order), and the largest difference of its output from (a)'s;
  (d) the traffic floor: 48 bytes per pixel and iteration (the X and G records in, the X record out) at the 6.3 TB/s
      HBM streams at, computed, not measured.
The child is a process of its own under a time limit, and a failure ends the run.  It prints the medians, the min..max
of the launches and the ratios; nothing asserts a time.
"""
import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
W, H, SPP, SEED, ITER = 1920, 1080, 4, 7, 5
SCENES = ("jumpy-balls",)
WARMUP, LAUNCHES, LIMIT_S = 2, 7, 500
HBM_BYTES_PER_S = 6.3e12
MASKS = ("0", "1", "2", "3", "4", "7")


def load_rtw(pkg):
    spec = importlib.util.spec_from_file_location("rtw_amd", pkg / "__init__.py", submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["rtw_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def torch_denoise(torch, sums, sq, albedo, normal, depth, n, iterations, sigma_l, sigma_n, sigma_z):
    """include/rtw.h's filter on [h, w, c] float32 tensors holding n samples per pixel -> mean radiance [h, w, 3]"""
    h, w = sums.shape[:2]
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=sums.device)  # noqa: E731
    zero, one = f(0.0), f(1.0)
    inv = one / f(float(n))
    m = sums * inv
    a = albedo * inv
    d = torch.where(a > 0.001, a, f(0.001))
    x = m / d
    v = sq * inv - m * m
    v = torch.where(v < 0, zero, v)
    u = (v * inv) / (d * d)
    var = (u[..., 0] + u[..., 1]) + u[..., 2]
    nn = (normal[..., 0] * normal[..., 0] + normal[..., 1] * normal[..., 1]) + normal[..., 2] * normal[..., 2]
    g = torch.where((nn > 0)[..., None], normal / torch.sqrt(nn)[..., None], zero)
    z = depth[..., 0] * inv
    k_n = one / (f(sigma_n) * f(sigma_n))
    hh = (0.375, 0.25, 0.0625)

    def max0(t):
        return torch.where(t > 0, t, zero)

    def lum(t):
        return (0.2126 * t[..., 0] + 0.7152 * t[..., 1]) + 0.0722 * t[..., 2]

    for k in range(iterations):
        step = 1 << k
        l = lum(x)
        rz = one / ((f(sigma_z) * f(float(step))) * torch.abs(z) + 1e-6)
        rl = one / (f(sigma_l) * torch.sqrt(var) + 1e-4)
        sw, sv, sx = torch.zeros_like(var), torch.zeros_like(var), torch.zeros_like(x)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * step, dx * step
                p = (slice(max(0, -oy), h - max(0, oy)), slice(max(0, -ox), w - max(0, ox)))
                q = (slice(max(0, oy), h - max(0, -oy)), slice(max(0, ox), w - max(0, -ox)))
                if p[0].start >= p[0].stop or p[1].start >= p[1].stop:
                    continue
                e = g[p] - g[q]
                dn2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                wt = (hh[abs(dx)] * hh[abs(dy)]) * max0(one - dn2 * k_n)
                wt = wt * max0(one - torch.abs(z[p] - z[q]) * rz[p])
                lq = l[q]
                wt = wt * max0(one - torch.abs(l[p] - lq) * rl[p])
                cnt = (wt > 0) & (lq == lq)
                sw[p] = torch.where(cnt, sw[p] + wt, sw[p])
                sx[p] = torch.where(cnt[..., None], sx[p] + wt[..., None] * x[q], sx[p])
                sv[p] = torch.where(cnt, sv[p] + (wt * wt) * var[q], sv[p])
        ok = sw > 0
        x = torch.where(ok[..., None], sx / sw[..., None], x)
        var = torch.where(ok, sv / (sw * sw), var)
    return x * d


def measure(name, pkg):
    import torch
    os.environ["RTW_TUNING"] = "1"
    rtw = load_rtw(pkg)
    s = rtw.Scene()
    cam, bg = s.preset(name, W / H, seed=42)
    s.commit(device=0)
    rt = rtw.Raytracer(s, cam, bg, W, H, SPP, seed=SEED)
    dev = "cuda:0"
    bufs = {k: torch.zeros((H, W, c), dtype=torch.float32, device=dev)
            for k, c in (("sums", 3), ("sq", 3), ("albedo", 3), ("normal", 3), ("depth", 2))}
    torch.cuda.synchronize()
    rt.render_samples_device(bufs["sums"].data_ptr(), bufs["sq"].data_ptr(), device=0)
    rt.render_features_device(bufs["albedo"].data_ptr(), bufs["normal"].data_ptr(), bufs["depth"].data_ptr(), device=0)
    torch.cuda.synchronize()
    out = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    scratch = torch.zeros(rtw.denoise_scratch_bytes(W, H), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = [bufs[k].data_ptr() for k in ("sums", "sq", "albedo", "normal", "depth")]
    sig = dict(sigma_l=rtw.DENOISE_SIGMA_L, sigma_n=rtw.DENOISE_SIGMA_N, sigma_z=rtw.DENOISE_SIGMA_Z)

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

    def hip(mask, iterations):
        if mask is None:
            os.environ.pop("RTW_DENOISE_LDS", None)
        else:
            os.environ["RTW_DENOISE_LDS"] = mask
        return timed(lambda: rtw.denoise_device(*ptrs, W, H, SPP, out.data_ptr(), scratch.data_ptr(),
                                                iterations=iterations, device=0, stream_ptr=stream, **sig))

    res = {"scene": name, "lib_sha": rtw.lib_sha(), "pixels": W * H, "iterations": ITER,
           "floor_ms": round(48.0 * W * H * ITER / HBM_BYTES_PER_S * 1e3, 4)}
    res["hip_ms"] = hip(None, ITER)
    mine = out.clone()
    res["hip_mask_ms"] = {m: hip(m, ITER) for m in MASKS}
    res["step1_ms"] = {m: hip(m, 1) for m in ("0", "1")}
    res["step2_ms"] = {m: hip(m, 2) for m in ("0", "2")}
    hip(None, ITER)
    res["hip_repeat_equal"] = bool(torch.equal(out.view(torch.int32), mine.view(torch.int32)))
    args = [bufs[k] for k in ("sums", "sq", "albedo", "normal", "depth")]
    res["torch_ms"] = timed(lambda: torch_denoise(torch, *args, SPP, ITER, *sig.values()))
    ref = torch_denoise(torch, *args, SPP, ITER, *sig.values())
    both = torch.isfinite(ref) & torch.isfinite(mine)
    res["torch_max_abs_diff"] = float((ref - mine)[both].abs().max().item())
    res["torch_bits_equal"] = bool(torch.equal(ref.view(torch.int32), mine.view(torch.int32)))
    print(json.dumps(res))


def mm(xs):
    return f"{np.median(xs):.3f} ms ({min(xs):.3f}..{max(xs):.3f})"


def show(res):
    a, t = np.median(res["hip_ms"]), np.median(res["torch_ms"])
    print(f"{res['scene']} {W}x{H}, {ITER} iterations; lib {res['lib_sha']}")
    print(f"  (a) rtw_denoise_device {mm(res['hip_ms'])}; repeat bit-equal {res['hip_repeat_equal']}")
    for m, xs in res["hip_mask_ms"].items():
        print(f"  (b) RTW_DENOISE_LDS={m}: {mm(xs)}")
    print(f"  (b) 1 iteration: global {mm(res['step1_ms']['0'])}, LDS {mm(res['step1_ms']['1'])}")
    print(f"  (b) 2 iterations, step 2: global {mm(res['step2_ms']['0'])}, LDS {mm(res['step2_ms']['2'])}")
    print(f"  (c) torch tensor ops {mm(res['torch_ms'])}; (a)/(c) {a / t:.4f}; output vs (a): bits equal "
          f"{res['torch_bits_equal']}, max |diff| {res['torch_max_abs_diff']:.3g}")
    print(f"  (d) traffic floor {res['floor_ms']:.3f} ms (48 B x {res['pixels']} px x {ITER} at 6.3 TB/s); "
          f"(a)/(d) {a / res['floor_ms']:.2f}", flush=True)


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
