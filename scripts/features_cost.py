#!/usr/bin/env python3
"""Cost of the feature buffers (rtw_render_features_device) beside the chain they replace and beside the colour samples
of the same frame: python scripts/features_cost.py [--pkg DIR] [--rounds N] [scene ...]

For jumpy-balls and wavefront-cow-obj at 1920x1080, 8 samples per pixel, it times three things by HIP events
(stats.kernel_ms; torch events around the torch part), 2 warm-ups and then 7 launches each:
  (a) rtw_render_features_device, all three buffers, samples [0, 8) onto zeroed device buffers;
  (b) the composed chain over the same samples: rtw_camera_rays_device -> rtw_hit_rays_device ->
      rtw_scatter_rays_device (three staging arrays of w*h*spp records) and a torch per-pixel sum of albedo, normal and
      (t, hit) over the sample axis; the chain's kernel times and the sum's are added, the gaps between them left out,
      in the chain's favour;
  (c) rtw_render_samples_device for the same 8 samples (max_depth 50), the colour frame the guides go with.
--pkg DIR loads the Python package (and the library built beside it) from DIR instead of this tree's
raytracer-weekend_amd: a build of an earlier commit, whose (b) and (c) are code the feature did not touch; (a) is left
out where the package has no render_features_device.  With --pkg the script runs `--rounds` rounds (default 2), each
round this tree's child and then DIR's child per scene, so that the two builds alternate on the same device.
Each child is a process of its own under a time limit, and a failure ends the run.  It prints the medians, the
min..max of the launches, and the ratios (a)/(b) and (a)/(c) of the medians; nothing asserts a time.
"""
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
W, H, SPP, MAX_DEPTH, SEED = 1920, 1080, 8, 50, 7
SCENES = ("jumpy-balls", "wavefront-cow-obj")
WARMUP, LAUNCHES, LIMIT_S = 2, 7, 400


def load_rtw(pkg):
    spec = importlib.util.spec_from_file_location("rtw_amd", pkg / "__init__.py", submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["rtw_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def chain(rtw, s, cam, bg, torch, bufs):
    """-> summed ms of camera_rays -> hit_rays -> scatter_rays and the torch per-pixel sums"""
    n = W * H * SPP
    d_rays, d_hits, d_out, d_sc = bufs
    ms = s.camera_rays_device(cam, W, H, SPP, SEED, 0, n, d_rays.data_ptr(), 0, 0, want_stats=True)["kernel_ms"]
    ms += s.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, 0, 0, want_stats=True)["kernel_ms"]
    ms += s.scatter_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), bg, d_out.data_ptr(), d_sc.data_ptr(), n, 0, 0,
                                want_stats=True)["kernel_ms"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    hf = d_hits.view(torch.float32).view(H * W, SPP, 12)  # p, normal, t, u | v, material, key, flags
    sf = d_sc.view(torch.float32).view(H * W, SPP, 8)     # attenuation, emitted, flags, reserved
    hit = (d_hits.view(torch.int32).view(H * W, SPP, 12)[..., 11] & rtw.HIT_HIT) != 0
    scattered = (d_sc.view(torch.int32).view(H * W, SPP, 8)[..., 6] & rtw.SCATTER_SCATTERED) != 0
    albedo = torch.where(scattered[..., None], sf[..., 0:3], sf[..., 3:6]).sum(dim=1)
    normal = torch.where(hit[..., None], hf[..., 3:6], torch.zeros((), device=hf.device)).sum(dim=1)
    depth = torch.stack([torch.where(hit, hf[..., 6], torch.zeros((), device=hf.device)), hit.float()], dim=-1).sum(dim=1)
    e1.record()
    torch.cuda.synchronize()
    assert albedo.shape == normal.shape == (H * W, 3) and depth.shape == (H * W, 2)
    return ms + e0.elapsed_time(e1)


def measure(name, pkg):
    import torch
    rtw = load_rtw(pkg)
    s = rtw.Scene()
    cam, bg = s.preset(name, W / H, seed=42)
    s.commit(device=0)
    n = W * H * SPP
    rt = rtw.Raytracer(s, cam, bg, W, H, SPP, seed=SEED, max_depth=MAX_DEPTH)
    dev = "cuda:0"
    res = {"scene": name, "pkg": str(pkg), "samples": n, "kernel": [s.info(k) for k in range(16, 24)],
           "lib_sha": rtw.lib_sha()}
    if hasattr(rt, "render_features_device"):
        fa, fn, fd = (torch.zeros(H * W * c, dtype=torch.float32, device=dev) for c in (3, 3, 2))
        ams = []
        for _ in range(WARMUP + LAUNCHES):
            for t in (fa, fn, fd):
                t.zero_()
            st = rt.render_features_device(fa.data_ptr(), fn.data_ptr(), fd.data_ptr(), 0, SPP, want_stats=True)
            assert st["rays"] == n, (st["rays"], n)
            ams.append(st["kernel_ms"])
        res["features_ms"] = [round(x, 4) for x in ams[WARMUP:]]
        res["hit_fraction"] = round(float(fd.view(H * W, 2)[:, 1].sum().item()) / n, 4)
    bufs = tuple(torch.zeros(n * b, dtype=torch.uint8, device=dev) for b in (40, 48, 40, 32))
    res["chain_ms"] = [round(chain(rtw, s, cam, bg, torch, bufs), 4) for _ in range(WARMUP + LAUNCHES)][WARMUP:]
    del bufs
    d_sum, d_sq = (torch.zeros(H * W * 3, dtype=torch.float32, device=dev) for _ in range(2))
    cms = []
    for _ in range(WARMUP + LAUNCHES):
        d_sum.zero_()
        d_sq.zero_()
        cms.append(rt.render_samples_device(d_sum.data_ptr(), d_sq.data_ptr(), 0, SPP, want_stats=True)["kernel_ms"])
    res["samples_ms"] = [round(x, 4) for x in cms[WARMUP:]]
    print(json.dumps(res))


def show(res, who):
    def mm(xs):
        return f"{np.median(xs):.3f} ms ({min(xs):.3f}..{max(xs):.3f})"
    line = f"{res['scene']} [{who}]: (b) chain {mm(res['chain_ms'])}; (c) colour samples {mm(res['samples_ms'])}"
    if "features_ms" in res:
        a = np.median(res["features_ms"])
        line = (f"{res['scene']} [{who}]: (a) features {mm(res['features_ms'])}, hit fraction {res['hit_fraction']}; " +
                line.split(": ", 1)[1] + f"; (a)/(b) {a / np.median(res['chain_ms']):.3f}, "
                f"(a)/(c) {a / np.median(res['samples_ms']):.3f}")
    print(line + f"; kernel cfg {res['kernel']}; lib {res['lib_sha']}", flush=True)


def child(name, pkg):
    r = subprocess.run([sys.executable, __file__, "--child", name, str(pkg)], timeout=LIMIT_S, capture_output=True,
                       text=True)
    if r.returncode != 0:
        sys.exit(f"{name} ({pkg}): exit status {r.returncode}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    args = sys.argv[1:]
    if len(args) == 3 and args[0] == "--child":
        return measure(args[1], Path(args[2]))
    other, rounds = None, 1
    while args and args[0] in ("--pkg", "--rounds"):
        if args[0] == "--pkg":
            other, rounds = Path(args[1]).resolve(), max(rounds, 2)
        else:
            rounds = int(args[1])
        args = args[2:]
    here = ROOT / "raytracer-weekend_amd"
    for k in range(rounds):
        for name in args or SCENES:
            mine = child(name, here)
            show(mine, f"this tree, round {k + 1}")
            if other:
                theirs = child(name, other)
                show(theirs, f"{other.name}, round {k + 1}")
                a = np.median(mine["features_ms"])
                print(f"  (a) this tree / (b) {other.name}: {a / np.median(theirs['chain_ms']):.3f}; "
                      f"(b) this tree / (b) {other.name}: "
                      f"{np.median(mine['chain_ms']) / np.median(theirs['chain_ms']):.3f}", flush=True)


if __name__ == "__main__":
    main()
