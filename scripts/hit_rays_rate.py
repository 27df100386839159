#!/usr/bin/env python3
"""Rate of the ray-query kernel (rtw_hit_rays_device) on primary rays, and of the scatter kernel
(rtw_scatter_rays_device) on their hit records: python scripts/hit_rays_rate.py [scene ...]

For jumpy-balls and wavefront-cow-obj at 1920x1080 it makes one primary ray per pixel on the host, once (the preset's
camera with lens and shutter samples from numpy, in the render's 8x8-tile order, so that a wave's 64 consecutive rays
are one tile), and times rtw_hit_rays_device over them by stats.kernel_ms: 5 launches after 2 warm-ups.  Each scene
runs in a child process of its own under a time limit, and a failure ends the run.  Beside the rate it prints the
same scene's path-kernel Mrays/s where BENCH_r06.json records one, as context only: primary rays are more coherent
than bounces, and a query neither shades nor regenerates, so the two are no pass / fail pair.  Nothing asserts a rate.

The rays carry non-zero stream words (drawn after everything else, so the rays themselves are the ones this script
always made), and after the query rtw_scatter_rays_device is timed the same way over the query's records: 2 warm-ups,
the median of 5 launches, HIP events.  It streams records, so it is reported as M records/s and as achieved bytes/s at
160 B per record (40 + 48 read, 40 + 32 written) beside the time that traffic takes at 6.29 TB/s, the measured
float4-copy rate of an MI355X.
"""
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
W, H = 1920, 1080
SCENES = ("jumpy-balls", "wavefront-cow-obj")
WARMUP, LAUNCHES, LIMIT_S = 2, 5, 240
RECORD_BYTES = 40 + 48 + 40 + 32  # scatter_kernel per record: rtw_ray + rtw_hit read, rtw_ray + rtw_scatter written
COPY_BYTES_PER_S = 6.29e12        # measured float4-copy rate of one MI355X


def load_rtw():
    pkg = ROOT / "raytracer-weekend_amd"
    spec = importlib.util.spec_from_file_location("rtw_amd", pkg / "__init__.py", submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["rtw_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def primary_rays(rtw, cam, rng):
    """camera.rs:66-74 for one sample per pixel, pixels in 8x8 tiles (tile-major, then row-major inside a tile)."""
    c = cam.as_dict()
    ty, tx, ly, lx = np.meshgrid(np.arange((H + 7) // 8), np.arange((W + 7) // 8), np.arange(8), np.arange(8),
                                 indexing="ij")
    i, row = (tx * 8 + lx).reshape(-1), (ty * 8 + ly).reshape(-1)
    keep = (i < W) & (row < H)
    i, j = i[keep], H - 1 - row[keep]
    n = len(i)
    u = ((i + rng.random(n)) / (W - 1))[:, None]
    v = ((j + rng.random(n)) / (H - 1))[:, None]
    r = np.sqrt(rng.random(n)) * c["lens_radius"]
    phi = rng.random(n) * 2 * np.pi
    off = np.array(c["u"]) * (r * np.cos(phi))[:, None] + np.array(c["v"]) * (r * np.sin(phi))[:, None]
    o = np.array(c["origin"]) + off
    d = np.array(c["lower_left_corner"]) + u * np.array(c["horizontal"]) + v * np.array(c["vertical"]) - o
    t = c["time0"] + rng.random(n) * (c["time1"] - c["time0"])
    streams = rng.integers(1, 1 << 63, n, dtype=np.uint64)  # (last: the draws above are the ones they always were)
    return rtw.make_rays(o, d, np.clip(t, c["time0"], c["time1"]), streams)


def measure(name):
    import torch
    rtw = load_rtw()
    s = rtw.Scene()
    cam, bg = s.preset(name, W / H, seed=42)
    s.commit(device=0)
    rays = primary_rays(rtw, cam, np.random.default_rng(1))
    n = len(rays)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).to("cuda:0")
    d_hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
    ms = [s.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, 0, 0, want_stats=True)["kernel_ms"]
          for _ in range(WARMUP + LAUNCHES)][WARMUP:]
    hits = np.frombuffer(d_hits.cpu().numpy().tobytes(), rtw.HIT_DTYPE)
    # the scatter kernel over the query's records (out of place: every launch reads the same input)
    d_out = torch.zeros(n * 40, dtype=torch.uint8, device="cuda:0")
    d_sc = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    sms = [s.scatter_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), bg, d_out.data_ptr(), d_sc.data_ptr(), n, 0, 0,
                                 want_stats=True)["kernel_ms"] for _ in range(WARMUP + LAUNCHES)][WARMUP:]
    sc = np.frombuffer(d_sc.cpu().numpy().tobytes(), rtw.SCATTER_DTYPE)
    smed = float(np.median(sms))
    print(json.dumps({"scene": name, "rays": n, "hit_fraction": float(((hits["flags"] & rtw.HIT_HIT) != 0).mean()),
                      "kernel_ms": [round(x, 4) for x in ms], "mrays_per_s": round(n / (np.median(ms) * 1e3), 1),
                      "scatter_ms": [round(x, 4) for x in sms], "scatter_mrec_per_s": round(n / (smed * 1e3), 1),
                      "scatter_tb_per_s": round(n * RECORD_BYTES / (smed * 1e-3) / 1e12, 3),
                      "scatter_bound_ms": round(n * RECORD_BYTES / COPY_BYTES_PER_S * 1e3, 4),
                      "scattered_fraction": float(((sc["flags"] & rtw.SCATTER_SCATTERED) != 0).mean()),
                      "kernel": [s.info(k) for k in range(16, 24)], "lib_sha": rtw.lib_sha()}))


def path_kernel_rate(name):
    try:
        p = json.loads((ROOT / "BENCH_r06.json").read_text())["parsed"]
        cfg = p["config"]
        if (cfg["scene"], cfg["width"], cfg["height"]) == (name, W, H):
            return f"{p['value']:.0f} {p['unit']} at {cfg['spp']} spp"
    except (OSError, KeyError, ValueError):
        pass
    return "not recorded"


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return measure(sys.argv[2])
    for name in sys.argv[1:] or SCENES:
        r = subprocess.run([sys.executable, __file__, "--child", name], timeout=LIMIT_S, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"{name}: exit status {r.returncode}\n{r.stderr[-2000:]}")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"{name}: {res['mrays_per_s']} Mrays/s over {res['rays']} primary rays ({res['hit_fraction']:.1%} hit; "
              f"kernel ms {res['kernel_ms']}; kernel cfg {res['kernel']}; lib {res['lib_sha']}); path kernel in "
              f"BENCH_r06.json: {path_kernel_rate(name)}", flush=True)
        print(f"{name}: scatter {res['scatter_mrec_per_s']} M records/s = {res['scatter_tb_per_s']} TB/s at "
              f"{RECORD_BYTES} B per record (kernel ms {res['scatter_ms']}; {res['scattered_fraction']:.1%} "
              f"scattered); "
              f"bound {res['scatter_bound_ms']} ms = {res['rays']} x {RECORD_BYTES} B / 6.29 TB/s", flush=True)


if __name__ == "__main__":
    main()
