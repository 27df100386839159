"""Random sphere worlds and cameras through the 1024-lane ring kernel, GPU vs oracle, bit for bit.

tests/test_sphere_fuzz_worlds.py draws the cases (world classes cluster, field, bare, dome, offset; camera classes near,
sky, border, far; frames with partial tiles, a single tile, strips one tile high or wide).  Every camera of a case is
rendered

  1. by the ring kernel with the per-tile lists (rtw_scene_info 24 must be 1 for near and sky cameras, 0 for far ones;
     a border camera's value is recorded),
  2. by the ring kernel under RTW_TILE_LISTS=0,
  3. by the plain sphere kernel (RTW_LDS_NODES=0: global nodes, per-lane starts),

and each frame must equal the ITERATIVE oracle's on uint32 views with the same ray count; (1) and (2) each other's.
Where the lists were used, the superset property is checked directly (4): every camera ray (rtw_camera_rays) whose
closest hit (rtw_hit_rays) is a BVH primitive finds it in its tile's record (rtw_diag_tile_lists), unless that tile is on
overflow.  (5) The records are kept per (camera, size, cap, stream): camera A, then camera B at A's frame size, then A
again must give A's first frame.  (6) For seed % 3 == 0 the frame is also rendered as two sample ranges
(rtw_render_samples_device) and as the in-order f32 sum of rtw_sample_rays' records over rtw_camera_rays.

RTW_SPHERE_FUZZ_SEEDS sets the number of seeds (default 35), RTW_SPHERE_FUZZ_FRAME=w,h,spp overrides every case's frame
for long offline runs.

Recorded runs (MI355X): this module's 36 tests (the 35 default seeds, 89 cameras, and the corpus test) take 4.7 s of
wall time, at most 0.34 s a seed; all are bit-exact.  Once, 1,000 seeds at RTW_SPHERE_FUZZ_FRAME=64,36,4 (2,591
cameras: 1,228 near, of which 683 with tiles on overflow, 369 sky, 517 border, 477 far; 84 s): 1,000 seeds run, 0
differing.  The host turned the lists on for 41 of the 517 border cameras (seeds 6 and 31 of the default range; half
the border cameras are aimed at the box's farthest corner for this: a lens of radius >= 0.5 otherwise straddles D0 by
far more than the 0.2 % the eye is placed within).  No product bug came out of these runs, so no seed is kept as a
named regression test.

What the tests are known to catch (mutations of a scratch build): with the camera compare removed from the lists
cache's key (frame_tile_lists) seeds 18 and 33 of the default range fail, the ones whose camera B is a near camera
(a sky camera's records are empty, and its rays miss under anybody's records).  BEAM_MARGIN and the `z1 < -az`
rejection are the business of tests/test_tile_beam.py, on the CPU: the BVH's leaf boxes are padded by 4e-5 of the
largest coordinate (pad_box), 20 times the beam test's f32 term at parameter 1, so no render can tell."""
import os

import numpy as np
import pytest

import test_sphere_fuzz_worlds as fw
from test_gpu_far import F_SPHERES, selected_kernel
from test_gpu_tile_lists import _same
from test_sphere_fuzz_worlds import BG, RING_KERNEL

pytestmark = pytest.mark.gpu

N_SEEDS = int(os.environ.get("RTW_SPHERE_FUZZ_SEEDS", str(fw.N_DEFAULT)))
FRAME = tuple(int(x) for x in os.environ["RTW_SPHERE_FUZZ_FRAME"].split(",")) \
    if os.environ.get("RTW_SPHERE_FUZZ_FRAME") else None
RESULTS = {}  # seed -> [(camera class, lists used, tiles on overflow, tiles)]: filled by the per-seed test


def _render(rtw, knobs, s, cam, w, h, spp, seed, depth, env=()):
    for k, v in env:
        knobs.setenv(k, v)
    kernel = selected_kernel(s)
    g, st = rtw.Raytracer(s, cam, BG, w, h, spp, seed=seed, max_depth=depth).render()
    used, over = s.info(24), s.info(25)
    for k, _v in env:
        knobs.delenv(k)
    return g, st["rays"], used, over, kernel


def _superset(rtw, s, cam, w, h, spp, seed, what):
    """(4): -> the number of camera rays whose closest hit is a BVH primitive on a tile with a list"""
    lists, _over, keys = rtw.diag_tile_lists(s, cam, w, h)
    prim_of_key = {int(k): p for p, k in enumerate(keys)}
    assert len(prim_of_key) == len(keys) == s.info(0) - s.info(5)
    rays = s.camera_rays(cam, w, h, spp, seed)
    hits = s.hit_rays(rays["origin"], rays["direction"], rays["time"], rays["stream"])
    p = np.arange(len(rays)) // spp  # p = (row * w + i) * spp + sample
    tile = (p // w // 8) * ((w + 7) // 8) + (p % w) // 8
    n = 0
    for q in np.flatnonzero(hits["flags"] & 1):
        prim = prim_of_key.get(int(hits["key"][q]))
        if prim is None or lists[tile[q]] is None:  # an always-tested giant; a tile on overflow: the start walks
            continue
        n += 1
        assert prim in lists[tile[q]], \
            f"{what}: path {q} (pixel {p[q] % w}, row {p[q] // w}, tile {tile[q]}) hits BVH primitive {prim}, " \
            f"not in its tile's list {lists[tile[q]]}"
    return n


def _two_ranges(rtw, s, cam, w, h, spp, seed, depth, a):
    import torch
    rt = rtw.Raytracer(s, cam, BG, w, h, spp, seed=seed, max_depth=depth)
    stream = torch.cuda.current_stream().cuda_stream
    d_sum = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    n_rays = 0
    for first, n in ((0, a), (a, spp - a)):
        st = rt.render_samples_device(d_sum.data_ptr(), 0, first, n, device=0, stream_ptr=stream, want_stats=True)
        n_rays += st["rays"]
    return d_sum.cpu().numpy(), n_rays


def _sample_sum(rtw, s, cam, w, h, spp, seed, depth):
    rays = s.camera_rays(cam, w, h, spp, seed)
    got = s.sample_rays(rays, BG, depth)
    assert not (got["flags"] & rtw.SAMPLE_BAD_RAY).any()
    with np.errstate(all="ignore"):
        pixel = np.zeros((h * w, 3), np.float32)
        Ls = got["color"].reshape(h * w, spp, 3)
        for k in range(spp):  # float32 throughout, in sample order, as reduce_kernel
            pixel = pixel + Ls[:, k]
    return pixel.reshape(h, w, 3), int(got["segments"].astype(np.uint64).sum())


def run_seed(rtw, orc, knobs, seed, frame=FRAME):
    """-> [(camera class, lists used, tiles on overflow, tiles)] of the seed's cameras, everything above asserted"""
    knobs.setenv("RTW_LIST_MAX", "0")  # read at commit
    knobs.delenv("RTW_TILE_LISTS", raising=False)
    _build, cams = fw.make_case(rtw, seed)
    s, _text, _imgs = fw.committed(rtw, seed, device=0)
    out, first = [], None
    for ci, (cam, cls, w, h, spp, depth) in enumerate(cams):
        if frame:
            w, h, spp = frame
        what = f"seed {seed} ({fw.CLASSES[seed % 5]}) camera {ci} ({cls}, {cam.tags}) {w}x{h}x{spp} depth {depth}"
        r, rays, _rays1 = fw.oracle_frame(rtw, orc, seed, ci, frame)
        # 1. the ring kernel with lists
        g, rays_g, used, over, kernel = _render(rtw, knobs, s, cam, w, h, spp, seed, depth)
        assert kernel == RING_KERNEL
        if cls in ("near", "sky"):
            assert used == 1, f"{what}: lists used = {used}"
        elif cls == "far":
            assert used == 0, f"{what}: lists used = {used}"
        _same(g, rays_g, r, rays, f"{what}: lists vs the oracle")
        out.append((cls, used, over, rtw.n_tiles(w, h)))
        # 2. without lists
        off, rays_off, used_off, _o, kernel = _render(rtw, knobs, s, cam, w, h, spp, seed, depth,
                                                      env=(("RTW_TILE_LISTS", "0"),))
        assert kernel == RING_KERNEL and used_off == 0
        _same(off, rays_off, r, rays, f"{what}: lists off vs the oracle")
        _same(g, rays_g, off, rays_off, f"{what}: lists vs lists off")
        # 3. the plain kernel: no LDS node table, so no ring and no lists
        pl, rays_pl, used_pl, _o, kernel = _render(rtw, knobs, s, cam, w, h, spp, seed, depth,
                                                   env=(("RTW_LDS_NODES", "0"),))
        assert kernel[3] == F_SPHERES and kernel[4] == 256 and kernel[5] == 0 and used_pl == 0, kernel
        _same(pl, rays_pl, r, rays, f"{what}: the plain kernel vs the oracle")
        # 4. the superset property, directly
        if used:
            _superset(rtw, s, cam, w, h, spp, seed, what)
        # 6. sample ranges and radiance queries
        if seed % 3 == 0:
            a = int(np.random.default_rng((3000 + seed, ci)).integers(0, spp + 1))
            two, rays_two = _two_ranges(rtw, s, cam, w, h, spp, seed, depth, a)
            _same(two, rays_two, g, rays_g, f"{what}: samples [0, {a}) + [{a}, {spp}) vs the frame")
            sm, rays_sm = _sample_sum(rtw, s, cam, w, h, spp, seed, depth)
            _same(sm, rays_sm, g, rays_g, f"{what}: summed rtw_sample_rays vs the frame")
        if ci == 0:
            first = (cam, w, h, spp, depth, g, rays_g, r, rays)
    # 5. the lists cache: A, then B at A's size, then A again
    cam_a, w, h, spp, depth, g_a, rays_a, r_a, rays_ra = first
    cam_b, cls_b, _w, _h, _spp, depth_b = cams[1]
    g, rays_g, used_a, _o, _k = _render(rtw, knobs, s, cam_a, w, h, spp, seed, depth)
    assert used_a == 1
    r_b, rays_rb, _ = fw.oracle_frame(rtw, orc, seed, 1, (w, h, spp))
    b, rays_b, _u, _o, _k = _render(rtw, knobs, s, cam_b, w, h, spp, seed, depth_b)
    _same(b, rays_b, r_b, rays_rb, f"seed {seed}: camera B ({cls_b}) at camera A's size vs the oracle")
    g2, rays_g2, used_a2, _o, _k = _render(rtw, knobs, s, cam_a, w, h, spp, seed, depth)
    assert used_a2 == 1
    _same(g2, rays_g2, g_a, rays_a, f"seed {seed}: camera A after camera B ({cls_b}) vs A's first frame")
    _same(g2, rays_g2, r_a, rays_ra, f"seed {seed}: camera A after camera B ({cls_b}) vs the oracle")
    return out


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_sphere_world_bit_exact(gpu, orc, knobs, seed):
    RESULTS[seed] = run_seed(gpu, orc, knobs, seed)


def test_corpus(gpu):
    """Over the default range: every seed ran; some near camera's frame had tiles on overflow at the default cap and
    some had none (both sides of the make step's "decided / walks" branch ran).  What the host decided for the border
    cameras is printed."""
    missing = [seed for seed in range(fw.N_DEFAULT) if seed not in RESULTS]
    assert not missing, f"seeds that did not run (or failed): {missing}"
    near = [(seed, used, over, nt) for seed in range(fw.N_DEFAULT) for cls, used, over, nt in RESULTS[seed]
            if cls == "near"]
    border = [(seed, used) for seed in range(fw.N_DEFAULT) for cls, used, _o, _n in RESULTS[seed] if cls == "border"]
    print(f"near (seed, lists, overflow tiles, tiles): {near}")
    print(f"border (seed, lists used): {border}")
    assert any(over > 0 for _s, _u, over, _n in near), "no near case had a tile on overflow"
    assert any(over == 0 for _s, _u, over, _n in near), "every near case had tiles on overflow"
