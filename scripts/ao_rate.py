#!/usr/bin/env python3
"""Cost of the fused ambient-occlusion pass (rtw_render_ao_device) beside the walks it contains and beside the unfused
chain it replaces: python scripts/ao_rate.py [scene ...]      (MI355X only; a measurement, not a test)

For jumpy-balls and wavefront-cow-obj at 1920x1080, 4 samples per pixel, with K = 1 and 4 AO rays per hit and a radius
of 2% of the scene diagonal and of +inf, it times three things by HIP events (stats.kernel_ms; torch events around the
torch parts), in alternation in one process per scene, 2 warm-up rounds and then 5 measured ones:
  (f) rtw_render_ao_device, samples [0, 4) onto a zeroed device buffer;
  (a) the floor: rtw_render_features_device (depth only) for the same samples plus rtw_occluded_rays_device over as many
      AO rays with the same bounds (the rays (b) made) -- the two walks the fused pass contains, without anything
      between them; the fused pass cannot beat it;
  (b) the unfused chain: rtw_camera_rays_device -> rtw_hit_rays_device -> a torch expression that makes the AO rays of
      the hits (direction normal + a uniform unit vector, K per hit, bound radius / |d|) into an rtw_ray[] ->
      rtw_occluded_rays_device -> a torch per-pixel sum of (open, cast); kernel times and torch times added, the gaps
      between them left out, in the chain's favour.
(b)'s rays are torch's draws, not the fused pass's: the same distribution from the same hits, so the same work within
noise; the (open, cast) totals of both are printed side by side.  The scene diagonal is that of the box around the
frame's first hits (jumpy-balls' own box is its r = 1000 ground sphere's).  It prints medians, min..max, the ratios
(f)/(a) and (f)/(b) and the AO rays per second of (f); nothing asserts a time.
"""
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
W, H, SPP, SEED = 1920, 1080, 4, 7
SCENES = ("jumpy-balls", "wavefront-cow-obj")
RAYS_PER_HIT = (1, 4)
WARMUP, ROUNDS, LIMIT_S = 2, 5, 400


def load_rtw(pkg):
    spec = importlib.util.spec_from_file_location("rtw_amd", pkg / "__init__.py", submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["rtw_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def measure(name):
    import torch
    rtw = load_rtw(ROOT / "raytracer-weekend_amd")
    s = rtw.Scene()
    cam, bg = s.preset(name, W / H, seed=42)
    s.commit(device=0)
    dev = "cuda:0"
    n = W * H * SPP
    rt = rtw.Raytracer(s, cam, bg, W, H, SPP, seed=SEED)
    d_rays = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
    d_hits = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
    d_ao = torch.zeros(H * W * 2, dtype=torch.float32, device=dev)
    d_depth = torch.zeros(H * W * 2, dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)

    def chain_front():
        ms = s.camera_rays_device(cam, W, H, SPP, SEED, 0, n, d_rays.data_ptr(), 0, 0, want_stats=True)["kernel_ms"]
        return ms + s.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, 0, 0, want_stats=True)["kernel_ms"]

    def make_rays(K, radius):
        """the AO rays of the hits as rtw_ray records (10 words each), their bounds and their pixels"""
        hf = d_hits.view(torch.float32).view(n, 12)  # p, normal, t, u | v, material, key, flags
        hit = (d_hits.view(torch.int32).view(n, 12)[:, 11] & rtw.HIT_HIT) != 0
        idx = hit.nonzero().squeeze(1).repeat_interleave(K)
        u = torch.randn((idx.numel(), 3), device=dev, generator=gen)
        d = hf[idx, 3:6] + u / u.norm(dim=1, keepdim=True)
        rec = torch.empty((idx.numel(), 10), dtype=torch.float32, device=dev)
        rec[:, 0:3] = hf[idx, 0:3]
        rec[:, 3:6] = d
        rec[:, 6] = d_rays.view(torch.float32).view(n, 10)[idx, 6]
        rec[:, 7] = 0.0
        rec.view(torch.int32)[:, 8:10] = torch.randint(1, 2 ** 31 - 1, (idx.numel(), 2), device=dev, generator=gen,
                                                       dtype=torch.int32)
        return rec, radius / d.norm(dim=1), idx // SPP

    def sums(occ, pixel, K):
        out = torch.zeros((H * W, 2), dtype=torch.float32, device=dev)
        out[:, 0].index_add_(0, pixel, (occ == 0).float())
        out[:, 1].index_add_(0, pixel, torch.ones_like(pixel, dtype=torch.float32))
        return out

    chain_front()
    p = d_hits.view(torch.float32).view(n, 12)
    p = p[(d_hits.view(torch.int32).view(n, 12)[:, 11] & rtw.HIT_HIT) != 0][:, 0:3]
    p = p[torch.isfinite(p).all(dim=1)]
    diag = float((p.max(dim=0).values - p.min(dim=0).values).norm().item())
    del p
    for K in RAYS_PER_HIT:
        for radius in (0.02 * diag, float("inf")):
            f_ms, a_ms, b_ms = [], [], []
            for _ in range(WARMUP + ROUNDS):
                d_ao.zero_()
                st = rtw.render_ao_device(s, cam, W, H, d_ao.data_ptr(), SPP, ao_rays=K, radius=radius, seed=SEED,
                                          want_stats=True)
                f_ms.append(st["kernel_ms"])
                fused = d_ao.view(H * W, 2).sum(dim=0, dtype=torch.float64).tolist()
                # (b) the chain
                ms = chain_front()
                (rec, t_max, pixel), t1 = timed(torch, lambda: make_rays(K, radius))
                occ = torch.zeros(rec.shape[0], dtype=torch.uint8, device=dev)
                ms_occ = s.occluded_rays_device(rec.data_ptr(), t_max.data_ptr(), occ.data_ptr(), rec.shape[0], 0, 0,
                                                want_stats=True)["kernel_ms"]
                out, t2 = timed(torch, lambda: sums(occ, pixel, K))
                b_ms.append(ms + t1 + ms_occ + t2)
                chain = out.sum(dim=0, dtype=torch.float64).tolist()
                # (a) the floor: the two walks alone, over as many rays
                d_depth.zero_()
                ms_feat = rt.render_features_device(0, 0, d_depth.data_ptr(), 0, SPP, want_stats=True)["kernel_ms"]
                a_ms.append(ms_feat + ms_occ)
                assert st["rays"] - st["paths"] == rec.shape[0] == int(fused[1]) == int(chain[1]), "as many AO rays"
                del rec, t_max, pixel, occ, out
            print(json.dumps({"scene": name, "K": K, "radius": radius, "ao_rays": st["rays"] - st["paths"],
                              "paths": st["paths"], "fused_open_cast": fused, "chain_open_cast": chain,
                              "fused_ms": f_ms[WARMUP:], "floor_ms": a_ms[WARMUP:], "chain_ms": b_ms[WARMUP:],
                              "kernel": [s.info(k) for k in range(16, 24)]}), flush=True)


def show(r):
    def mm(xs):
        return f"{np.median(xs):.3f} ms ({min(xs):.3f}..{max(xs):.3f})"
    f, a, b = (np.median(r[k]) for k in ("fused_ms", "floor_ms", "chain_ms"))
    print(f"{r['scene']} K={r['K']} radius {r['radius']:.4g}: (f) fused {mm(r['fused_ms'])}, "
          f"{(r['ao_rays'] + r['paths']) / f / 1e3:.0f} Mrays/s ({r['ao_rays']} AO rays of {r['paths']} samples); "
          f"(a) floor {mm(r['floor_ms'])}; (b) chain {mm(r['chain_ms'])}; (f)/(a) {f / a:.3f}, (f)/(b) {f / b:.3f}; "
          f"open/cast fused {r['fused_open_cast'][0] / max(r['fused_open_cast'][1], 1):.4f}, "
          f"chain {r['chain_open_cast'][0] / max(r['chain_open_cast'][1], 1):.4f}; kernel cfg {r['kernel']}", flush=True)


def main():
    args = sys.argv[1:]
    if len(args) == 2 and args[0] == "--child":
        return measure(args[1])
    for name in args or SCENES:
        r = subprocess.run([sys.executable, __file__, "--child", name], timeout=LIMIT_S, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"{name}: exit status {r.returncode}\n{r.stderr[-2000:]}")
        for ln in r.stdout.strip().splitlines():
            show(json.loads(ln))


if __name__ == "__main__":
    main()
