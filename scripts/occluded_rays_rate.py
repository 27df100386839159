#!/usr/bin/env python3
"""Rate of the occlusion-query kernel (rtw_occluded_rays_device) against the route it replaces, rtw_hit_rays_device
followed by a compare: python scripts/occluded_rays_rate.py [scene ...]

For jumpy-balls and wavefront-cow-obj at 1920x1080, three ray sets, each timed by stats.kernel_ms (HIP events), 2
warm-ups and the median of 5 launches:
  (a) primary  scripts/hit_rays_rate.py's primary rays, one per pixel in 8x8-tile order, no bounds (t_max = NULL):
               the occlusion kernel beside hit_kernel on the same rays.
  (b) ao       ambient-occlusion rays from the primary hits, origin p + 1e-3 n, cosine-hemisphere directions about n
               drawn by numpy (unit length), with t_max = 2% of the diagonal of the primary hit points' bounding box,
               and with t_max = +inf.
  (c) shadow   rays from the same origins to one point above the scene (the box's centre raised by its diagonal),
               unit directions, t_max = the distance.
For (b) and (c) the route it is compared with is hit_kernel's time on the same rays plus a torch compare
`hit & ~(t > T)` over the records, timed with torch events the same way.  `differ` counts the rays on which the two
routes disagree (0 expected: the kernel's contract).  Each scene runs in a child process of its own under a time limit,
and a failure ends the run.  Nothing asserts a rate."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from hit_rays_rate import H, SCENES, W, load_rtw, primary_rays  # noqa: E402

WARMUP, LAUNCHES, LIMIT_S = 2, 5, 300


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def secondary_rays(rtw, rays, hits, rng):
    """-> (ao rays, shadow rays, shadow distances, the hit points' diagonal) from the primary hits"""
    hit = (hits["flags"] & rtw.HIT_HIT) != 0
    p, n = hits["p"][hit].astype(np.float64), _unit(hits["normal"][hit].astype(np.float64))
    o = p + 1e-3 * n
    m = len(o)
    # cosine-weighted hemisphere about n: a unit-disk point lifted, in a frame built from n
    r, phi = np.sqrt(rng.random(m)), rng.random(m) * 2 * np.pi
    a = np.where(np.abs(n[:, :1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    t1 = _unit(np.cross(n, a))
    t2 = np.cross(n, t1)
    d = (r * np.cos(phi))[:, None] * t1 + (r * np.sin(phi))[:, None] * t2 + np.sqrt(1.0 - r * r)[:, None] * n
    lo, hi = p.min(axis=0), p.max(axis=0)
    diag = float(np.linalg.norm(hi - lo))
    light = 0.5 * (lo + hi) + np.array([0.0, diag, 0.0])
    to = light - o
    dist = np.linalg.norm(to, axis=1)
    time, stream = rays["time"][hit], rays["stream"][hit]
    return (rtw.make_rays(o, _unit(d), time, stream), rtw.make_rays(o, to / dist[:, None], time, stream),
            dist.astype(np.float32), diag)


def measure(name):
    import torch
    rtw = load_rtw()
    dev = torch.device("cuda:0")
    s = rtw.Scene()
    cam, _bg = s.preset(name, W / H, seed=42)
    s.commit(device=0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    med = lambda f: float(np.median([f() for _ in range(WARMUP + LAUNCHES)][WARMUP:]))

    def compare_ms(d_hits, d_T, d_out):
        rec = d_hits.view(torch.float32).view(-1, 12)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        flag = (rec[:, 11].view(torch.int32) & 1) != 0
        d_out.copy_((flag & ~(rec[:, 6] > d_T)) if d_T is not None else flag)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def one(rays, T):
        n = len(rays)
        d_rays, d_hits = up(rays), torch.zeros(n * 48, dtype=torch.uint8, device=dev)
        d_T = torch.from_numpy(np.ascontiguousarray(T, np.float32)).to(dev) if T is not None else None
        d_occ, d_cmp = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
        tp = d_T.data_ptr() if d_T is not None else 0
        occ = med(lambda: s.occluded_rays_device(d_rays.data_ptr(), tp, d_occ.data_ptr(), n, 0, 0,
                                                 want_stats=True)["kernel_ms"])
        hit = med(lambda: s.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, 0, 0, want_stats=True)["kernel_ms"])
        cmp_ms = med(lambda: compare_ms(d_hits, d_T, d_cmp))
        return {"rays": n, "occluded_ms": round(occ, 4), "hit_ms": round(hit, 4), "compare_ms": round(cmp_ms, 4),
                "occluded_mrays_per_s": round(n / (occ * 1e3), 1), "hit_mrays_per_s": round(n / (hit * 1e3), 1),
                "ratio_to_hit_then_compare": round((hit + cmp_ms) / occ, 3),
                "occluded_fraction": round(float((d_occ == 1).float().mean()), 4),
                "differ": int((d_occ != d_cmp).sum())}, d_hits

    prim = primary_rays(rtw, cam, np.random.default_rng(1))
    res = {"scene": name, "kernel": [s.info(k) for k in range(16, 24)], "lib_sha": rtw.lib_sha()}
    res["primary"], d_hits = one(prim, None)
    hits = np.frombuffer(d_hits.cpu().numpy().tobytes(), rtw.HIT_DTYPE)
    ao, shadow, dist, diag = secondary_rays(rtw, prim, hits, np.random.default_rng(2))
    res["diagonal"] = round(diag, 3)
    res["ao_2pct"] = one(ao, np.full(len(ao), 0.02 * diag, np.float32))[0]
    res["ao_inf"] = one(ao, np.full(len(ao), np.inf, np.float32))[0]
    res["shadow"] = one(shadow, dist)[0]
    print(json.dumps(res))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return measure(sys.argv[2])
    for name in sys.argv[1:] or SCENES:
        r = subprocess.run([sys.executable, __file__, "--child", name], timeout=LIMIT_S, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"{name}: exit status {r.returncode}\n{r.stderr[-2000:]}")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"{name}: kernel cfg {res['kernel']}; lib {res['lib_sha']}; hit points' diagonal {res['diagonal']}",
              flush=True)
        for what in ("primary", "ao_2pct", "ao_inf", "shadow"):
            q = res[what]
            print(f"{name} {what}: occluded {q['occluded_mrays_per_s']} Mrays/s ({q['occluded_ms']} ms, {q['rays']} rays, "
                  f"{q['occluded_fraction']:.1%} occluded); hit_kernel {q['hit_mrays_per_s']} Mrays/s ({q['hit_ms']} ms) + "
                  f"compare {q['compare_ms']} ms: {q['ratio_to_hit_then_compare']} x; differ {q['differ']}", flush=True)


if __name__ == "__main__":
    main()
