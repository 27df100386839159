"""Full-resolution parity on every BASELINE.json GPU config.

Each config renders at its real resolution and camera (bench.py's CONFIGS: jumpy-balls
1920x1080, cornell-box 800x800, wavefront-cow-obj 1920x1080, textured-monument 3840x2160) at
1-2 spp.  The GPU renders a strided subset of 8-row tile bands through rtw_render_device (tile ids,
packed output); the oracle renders the same rows with the flat-list closest hit of
hittable/mod.rs:57-69 (a BvhNode group evaluated as the list of its leaves: set semantics).  The
sums must be bit-identical and the ray counts equal: this pins the kernel's BVH culling (padded
boxes, relative t slack, rcp slab test: rtw_flatten.cpp, rtw_dev_trace.hpp trace_run) on the
headline frames, not only on the small parity images.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FULLRES = [
    # config, scene, w, h, spp, tile-row bands
    ("jumpy-1080p", "jumpy-balls", 1920, 1080, 2, [0, 27, 54, 67, 81, 108, 134]),
    ("cornell-800", "cornell-box", 800, 800, 2, [0, 13, 26, 39, 50, 62, 75, 88, 99]),
    ("cow-1080p", "wavefront-cow-obj", 1920, 1080, 2, [0, 40, 60, 67, 75, 100, 134]),
    ("monument-4k", "textured-monument", 3840, 2160, 1, [0, 90, 135, 180, 269]),
]
SCENE_SEED, RENDER_SEED = 42, 2024  # bench.py's seeds: the benchmarked frame itself


@pytest.mark.parametrize("cfg,name,w,h,spp,bands", FULLRES, ids=[c[0] for c in FULLRES])
def test_fullres_bands_bit_exact(gpu, orc, cfg, name, w, h, spp, bands):
    torch = pytest.importorskip("torch")
    rtw = gpu
    s = rtw.Scene()
    cam, bg = s.preset(name, rtw.camera_aspect(w, h), seed=SCENE_SEED)
    text, imgs = s.dump(), s.images()
    s.commit(device=0)
    tx = (w + 7) // 8
    ids = np.concatenate([np.arange(b * tx, (b + 1) * tx) for b in bands]).astype(np.int32)
    d_ids = torch.tensor(ids, device="cuda:0")
    packed = torch.zeros((len(ids), 64, 3), dtype=torch.float32, device="cuda:0")
    rt = rtw.Raytracer(s, cam, bg, w, h, spp, seed=RENDER_SEED)
    st = rt.render_device(packed.data_ptr(), 0, d_ids.data_ptr(), len(ids),
                          torch.cuda.current_stream().cuda_stream, want_stats=True)
    g = packed.cpu().numpy()
    # output rows of the bands; the oracle takes j = h - 1 - row (lib.rs:58 order)
    rows = np.concatenate([np.arange(8 * b, min(h, 8 * b + 8)) for b in bands])
    o = orc.OracleScene(text, imgs)
    ref, rays = o.render(orc.camera_from_fields(cam.as_dict()), bg, w, h, spp, seed=RENDER_SEED,
                         threads=min(256, os.cpu_count() or 1), rows=[h - 1 - int(r) for r in rows])
    # packed [slot][lane] -> (row, col): slot = band k * tx + tile column, lane = 8 (row % 8) + col % 8
    got = np.zeros_like(ref)
    for k, b in enumerate(bands):
        blk = g[k * tx:(k + 1) * tx].reshape(tx, 8, 8, 3)          # [tile col][row % 8][col % 8]
        band = blk.transpose(1, 0, 2, 3).reshape(8, tx * 8, 3)      # [row % 8][col]
        r0, r1 = 8 * b, min(h, 8 * b + 8)
        got[r0:r1] = band[:r1 - r0, :w]
    assert st["rays"] == rays, f"{cfg}: ray count {st['rays']} vs oracle {rays}"
    sel = got[rows].view(np.uint32) != ref[rows].view(np.uint32)
    assert not sel.any(), f"{cfg}: {int(sel.sum())} mismatching components of {sel.size}"
    assert rays > len(rows) * w * spp  # every pixel traced at least its camera ray


def test_render_multi_single_gpu_equals_render(gpu):
    """rtw_render_multi (C-ABI multi-device path: tiles dealt to devices, RCCL send/recv gather to
    device 0) at n_gpus = 1 — the box leases one GPU — and n_gpus = 0 (every visible device): the
    frame and the ray count equal rtw_render's bit for bit; a second call reuses the cached
    communicator and buffers."""
    rtw = gpu
    s = rtw.Scene()
    cam, bg = s.preset("jumpy-balls", 16 / 9, seed=3)
    s.commit()
    rt = rtw.Raytracer(s, cam, bg, 72, 40, 3, seed=9)  # ragged: 9 x 5 tiles
    ref, st = rt.render()
    for n in (1, 0, 1):
        got, st2 = rt.render_multi(n)
        assert st2["rays"] == st["rays"]
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), n
    with pytest.raises(rtw.RtwError):
        rt.render_multi(rtw.device_count() + 1)


def test_render_reuses_buffers(gpu):
    """rtw_render keeps its device image buffer and events per scene copy: a sequence of
    frames (console_app's 30-camera animation) renders identically frame after frame."""
    rtw = gpu
    s = rtw.Scene()
    cam, bg = s.preset("cornell-box", 1.0, seed=3)
    s.commit()
    a, _ = rtw.Raytracer(s, cam, bg, 24, 24, 2, seed=1).render()
    b, _ = rtw.Raytracer(s, cam, bg, 16, 16, 2, seed=1).render()  # smaller frame in the same buffer
    c, _ = rtw.Raytracer(s, cam, bg, 24, 24, 2, seed=1).render()
    assert b.shape == (16, 16, 3)
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


def test_checker_extreme_arguments_bit_exact(gpu, orc):
    """Checker::value (texture.rs:69-81) at |f x| >= 65536 (exact integer pi reduction) and
    |f x| < 2^-12 (sinf x == x), beside the double fast path: GPU == oracle (glibc sinf)."""
    rtw = gpu
    s = rtw.Scene()
    white, black = s.solid_rgb(0.9, 0.9, 0.9), s.solid_rgb(0.1, 0.2, 0.1)
    big = s.lambertian(s.checker(black, white, 1.0e5))     # |f x| up to ~1e7
    tiny = s.lambertian(s.checker(white, black, 1.0e-8))   # |f x| < 2^-12 everywhere
    mixed = s.lambertian(s.checker(black, white, 3.0e4))   # all three ranges on one sphere
    s.sphere((0, -1000, 0), 1000, big)
    s.sphere((0, 1, 0), 1, tiny)
    s.sphere((-2.2, 1, 0), 1, mixed)
    s.sphere((2.2, 1, 0), 1, big)
    text = s.dump()
    s.commit()
    cam = rtw.Camera.new((0, 2, 9), (0, 1, 0), (0, 1, 0), 40, 16 / 9, 0.0, 9.0)
    w, h, spp = 64, 36, 3
    g, st = rtw.Raytracer(s, cam, (0.7, 0.8, 1.0), w, h, spp, seed=5).render()
    r, rays = orc.OracleScene(text).render(orc.camera_from_fields(cam.as_dict()), (0.7, 0.8, 1.0), w, h, spp,
                                           seed=5)
    assert st["rays"] == rays
    assert np.array_equal(g.view(np.uint32), r.view(np.uint32))


@pytest.mark.parametrize("name,w,h,spp", [("cornell-box", 800, 800, 32), ("jumpy-balls", 1920, 1080, 8)],
                         ids=["cornell-800x32", "jumpy-1080px8"])
def test_whole_frame_bit_exact(gpu, orc, name, w, h, spp):
    """Every pixel of a whole benchmark frame (bench.py's scene and seeds, reduced spp) against the oracle, bit for
    bit, and the frame's ray count (scripts/fullframe_parity.py, profiles/r05/fullframe).  cornell's 32 samples
    hold two in-plane bounces (NaN hits): exact.  jumpy's 8 samples hold one path with a far-origin
    spurious sphere hit: round 5's BVH culled it (23 more segments on the GPU); the far-origin walk
    of round 6 finds it, so the counts are equal."""
    rtw = gpu
    s = rtw.Scene()
    cam, bg = s.preset(name, w / h, seed=SCENE_SEED)
    text, imgs = s.dump(), s.images()
    s.commit()
    g, st = rtw.Raytracer(s, cam, bg, w, h, spp, seed=RENDER_SEED).render()
    r, rays = orc.OracleScene(text, imgs).render(orc.camera_from_fields(cam.as_dict()), bg, w, h, spp,
                                                seed=RENDER_SEED)
    bad = np.argwhere((g.view(np.uint32) != r.view(np.uint32)).any(axis=2))
    assert bad.size == 0, f"{len(bad)} mismatching pixels, first {bad[:4].tolist()}"
    assert int(st["rays"]) == int(rays)
