#!/usr/bin/env python3
"""Rate of the radiance-query kernel (rtw_sample_rays_device) on a frame's camera rays, beside the same frame's render
and the composed device loop: python scripts/sample_rays_rate.py [scene ...]

For jumpy-balls, cornell-box and wavefront-cow-obj it makes the camera rays of a 1920x1080x1 frame on the device
(rtw_camera_rays_device; the output's row-major order, so a wave's 64 consecutive rays are 64 neighbours of one image
row, not the render's 8x8 tile) and times rtw_sample_rays_device over them by stats.kernel_ms: 2 warm-ups, then the
median of 5 launches.  It prints the sum of the records' segments / that time beside two figures from the same process:
  (a) the same frame through rtw_render_device: stats.rays / stats.kernel_ms (path kernel + reduction), timed alike;
  (b) the composed device loop over max_depth bounces, rtw_hit_rays_device -> rtw_scatter_rays_device in place with
      the survivors compacted by torch between bounces: its rays / the sum of the two kernels' kernel_ms, which leaves
      the compaction and the launches' gaps out, in the loop's favour; one warm-up pass, then the median of 3.
Each scene runs in a child process of its own under a time limit, and a failure ends the run.  The three ray counts
must agree (they are the same paths); nothing asserts a rate.
"""
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
W, H, SPP, MAX_DEPTH, SEED = 1920, 1080, 1, 50, 7
SCENES = ("jumpy-balls", "cornell-box", "wavefront-cow-obj")
WARMUP, LAUNCHES, LIMIT_S = 2, 5, 300


def load_rtw():
    pkg = ROOT / "raytracer-weekend_amd"
    spec = importlib.util.spec_from_file_location("rtw_amd", pkg / "__init__.py", submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["rtw_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def composed(rtw, s, bg, d_rays0, n, torch):
    """-> (rays traced, summed kernel ms) of hit -> scatter over max_depth bounces with compaction"""
    rays = d_rays0.clone().view(n, 40)
    hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
    sc = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    traced, ms = 0, 0.0
    for _depth in range(MAX_DEPTH):
        m = rays.shape[0]
        if m == 0:
            break
        ms += s.hit_rays_device(rays.data_ptr(), hits.data_ptr(), m, 0, 0, want_stats=True)["kernel_ms"]
        ms += s.scatter_rays_device(rays.data_ptr(), hits.data_ptr(), bg, rays.data_ptr(), sc.data_ptr(), m, 0, 0,
                                    want_stats=True)["kernel_ms"]
        traced += m
        alive = (sc[:m * 32].view(m, 32)[:, 24] & rtw.SCATTER_SCATTERED) != 0  # flags' low byte
        rays = rays[alive].contiguous()
    return traced, ms


def measure(name):
    import torch
    rtw = load_rtw()
    s = rtw.Scene()
    cam, bg = s.preset(name, W / H, seed=42)
    s.commit(device=0)
    n = W * H * SPP
    d_rays = torch.zeros(n * 40, dtype=torch.uint8, device="cuda:0")
    s.camera_rays_device(cam, W, H, SPP, SEED, 0, n, d_rays.data_ptr(), 0, 0)
    d_out = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    st = [s.sample_rays_device(d_rays.data_ptr(), bg, MAX_DEPTH, d_out.data_ptr(), n, 0, 0, want_stats=True)
          for _ in range(WARMUP + LAUNCHES)][WARMUP:]
    rec = np.frombuffer(d_out.cpu().numpy().tobytes(), rtw.SAMPLE_DTYPE)
    segments = int(rec["segments"].astype(np.uint64).sum())
    assert all(x["rays"] == segments for x in st), (segments, [x["rays"] for x in st])
    d_img = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0")
    rt = rtw.Raytracer(s, cam, bg, W, H, SPP, seed=SEED, max_depth=MAX_DEPTH)
    rst = [rt.render_device(d_img.data_ptr(), 0, want_stats=True) for _ in range(WARMUP + LAUNCHES)][WARMUP:]
    loops = [composed(rtw, s, bg, d_rays, n, torch) for _ in range(1 + 3)][1:]
    assert rst[0]["rays"] == segments == loops[0][0], (rst[0]["rays"], segments, loops[0][0])
    sms, rms, lms = [x["kernel_ms"] for x in st], [x["kernel_ms"] for x in rst], [x[1] for x in loops]
    print(json.dumps({"scene": name, "paths": n, "segments": segments,
                      "sample_ms": [round(x, 4) for x in sms], "render_ms": [round(x, 4) for x in rms],
                      "composed_ms": [round(x, 4) for x in lms],
                      "sample_mrays_per_s": round(segments / (np.median(sms) * 1e3), 1),
                      "render_mrays_per_s": round(segments / (np.median(rms) * 1e3), 1),
                      "composed_mrays_per_s": round(segments / (np.median(lms) * 1e3), 1),
                      "kernel": [s.info(k) for k in range(16, 24)], "lib_sha": rtw.lib_sha()}))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return measure(sys.argv[2])
    for name in sys.argv[1:] or SCENES:
        r = subprocess.run([sys.executable, __file__, "--child", name], timeout=LIMIT_S, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"{name}: exit status {r.returncode}\n{r.stderr[-2000:]}")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"{name}: {res['paths']} paths, {res['segments']} segments; fused query {res['sample_mrays_per_s']} "
              f"Mrays/s (kernel ms {res['sample_ms']}); (a) render {res['render_mrays_per_s']} Mrays/s (kernel ms "
              f"{res['render_ms']}); (b) composed loop {res['composed_mrays_per_s']} Mrays/s (summed kernel ms "
              f"{res['composed_ms']}); kernel cfg {res['kernel']}; lib {res['lib_sha']}", flush=True)


if __name__ == "__main__":
    main()
