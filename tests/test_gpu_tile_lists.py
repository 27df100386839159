"""Camera rays resolved at ring make from per-tile primitive lists (rtw_tile_beam.h, tile_list_kernel,
path_kernel's start_decide, K.ldsn_ring()).

Once per render a small kernel lists, for every 8x8 tile, the BVH primitives a camera ray of the tile can possibly hit;
the ring's make step folds the always-list and that list with the walk's own sphere test, and a lane that takes the
entry starts with its first hit decided.  The lists only cull, so every frame and ray count here must equal, bit for
bit, the ITERATIVE oracle's and the same build's under RTW_TILE_LISTS=0.  Every case asserts the ring kernel's
configuration tuple (rtw_scene_info 16-23) and what rtw_scene_info 24 / 25 report of the render: lists used, tiles on
overflow.

The world: the r = 1000 ground in the always-list and 16 BVH spheres, of which 12 form the cluster the cameras look
at -- a glass ball with a negative-radius shell inside it, two coincident balls of different materials (the tie
rule), four moving and four static balls -- and 4 lie behind every camera.  (The flattener keeps a world of at most 16
leaves in one tree without an always-list, so 1 + 16 leaves is the smallest world with the ground outside the BVH; the
cluster of 12 is what a tile's list can hold, under the cap of 15, and every case meant to exercise the lists asserts 0
overflow tiles.)  RTW_LIST_MAX=0 keeps the world out of list mode."""
import numpy as np
import pytest

from test_gpu_far import F_SPHERES, selected_kernel

pytestmark = pytest.mark.gpu

BG = (0.7, 0.8, 1.0)
SEED = 9
RING_KERNEL = (16, 0, 8, F_SPHERES, 1024, 144, 0, 0)
# the "instant" shutter [0.25, 0.25]: Camera::new needs time0 < time1 (the reference's gen_range panics on an empty
# range, and rtw_camera_new refuses it), so its end is the next float above 0.25, the narrowest shutter there is
INSTANT_T1 = float(np.nextafter(np.float32(0.25), np.float32(1.0)))

_WORLDS = {}
_ORACLE = {}  # (swap, camera name, w, h, spp) -> (frame, rays): rendered once, shared, never written


def _world(rtw, knobs, swap=False):
    """-> (committed scene, text, images).  swap: the coincident pair in the other order."""
    knobs.setenv("RTW_LIST_MAX", "0")  # read at commit
    if swap not in _WORLDS:
        s = rtw.Scene()
        rng = np.random.default_rng(4)
        ground = s.lambertian(s.checker(s.solid_rgb(0.2, 0.3, 0.1), s.solid_rgb(0.9, 0.9, 0.9), 10.0))
        s.sphere((0, -1000, 0), 1000, ground)
        glass, red, steel = s.dielectric(1.5), s.lambertian_solid((0.8, 0.1, 0.1)), s.metal((0.7, 0.7, 0.9), 0.0)
        s.sphere((0, 0.5, 0), 0.5, glass)
        s.sphere((0, 0.5, 0), -0.45, glass)  # the hollow shell (scenes.rs' negative radius)
        for m in ((steel, red) if swap else (red, steel)):  # coincident: the later one wins the tie
            s.sphere((1.0, 0.3, 0.6), 0.3, m)
        mats = [s.lambertian_solid(tuple(rng.uniform(0.1, 0.9, 3))) for _ in range(3)] + [s.metal((0.8, 0.6, 0.2), 0.3)]
        for k in range(4):  # static
            s.sphere((-1.2 + 0.8 * k, 0.2, -0.9 + 0.3 * k), 0.2, mats[k])
        for k in range(4):  # moving over the committed shutter [0, 1]
            c0 = (-1.0 + 0.7 * k, 0.2, 1.1 + 0.2 * k)
            s.moving_sphere(c0, 0.0, (c0[0], 0.2 + 0.1 * (k + 1), c0[2]), 1.0, 0.2, mats[3 - k])
        for k in range(4):  # behind every camera of this file
            s.sphere((21.0 + k, 0.2, 6.0 - k), 0.2, mats[k])
        text, imgs = s.dump(), s.images()
        s.commit(device=0)
        _WORLDS[swap] = (s, text, imgs)
    s = _WORLDS[swap][0]
    assert s.info(5) == 1 and s.info(14) == 1  # the ground alone in the always-list; the far bound is on
    return _WORLDS[swap]


def _camera(rtw, name):
    new = rtw.Camera.new
    return {
        "preset": lambda: new((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 16 / 9, 0.1, 10.0, 0.0, 1.0),
        "pinhole": lambda: new((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 16 / 9, 0.0, 10.0, 0.0, 1.0),
        "wide_lens": lambda: new((9, 1.5, 2), (0, 0.3, 0), (0, 1, 0), 30.0, 16 / 9, 1.0, 9.0, 0.0, 1.0),
        "inside": lambda: new((0.45, 0.35, 0.2), (-3, 0.2, 0.4), (0, 1, 0), 90.0, 1.0, 0.1, 1.0, 0.0, 1.0),
        "down": lambda: new((0.2, 6.0, 0.3), (0.2, 0.0, 0.3), (0, 0, -1), 40.0, 1.0, 0.1, 5.8, 0.0, 1.0),
        "instant": lambda: new((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 16 / 9, 0.1, 10.0, 0.25, INSTANT_T1),
        # lens radius 0.5 focused 2 units away: at the cluster, 13 units away, a pixel's beam is ~6 units wide
        "blurred": lambda: new((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 16 / 9, 1.0, 2.0, 0.0, 1.0),
        "far": lambda: new((0.35, -1200.0, 0.15), (0.0, 0.2, 0.0), (1, 0, 0), 0.8, 1.0, 0.0, 1200.0, 0.0, 1.0),
    }[name]()


def _oracle(orc, text, imgs, swap, cam_name, cam, w, h, spp):
    key = (swap, cam_name, w, h, spp)
    if key not in _ORACLE:
        r, rays = orc.OracleScene(text, imgs).render(orc.camera_from_fields(cam.as_dict()), BG, w, h, spp, seed=SEED,
                                                     integrator=orc.ITERATIVE)
        r.setflags(write=False)
        _ORACLE[key] = (r, rays)
    return _ORACLE[key]


def _same(g, rays_g, r, rays, what):
    assert rays_g == rays, f"{what}: ray count {rays_g} vs {rays}"
    bad = np.argwhere((g.view(np.uint32) != r.view(np.uint32)).any(axis=2))
    assert bad.size == 0, f"{what}: {len(bad)} mismatching pixels, first {bad[:4].tolist()}: " \
                          f"{g[tuple(bad[0])]} vs {r[tuple(bad[0])]}"


def _render(rtw, knobs, s, cam, w, h, spp, lists=True):
    if lists:
        knobs.delenv("RTW_TILE_LISTS", raising=False)
    else:
        knobs.setenv("RTW_TILE_LISTS", "0")
    assert selected_kernel(s) == RING_KERNEL
    g, st = rtw.Raytracer(s, cam, BG, w, h, spp, seed=SEED).render()
    used, over = s.info(24), s.info(25)
    knobs.delenv("RTW_TILE_LISTS", raising=False)
    return g, st["rays"], used, over


def _check(rtw, orc, knobs, cam_name, w, h, spp, expect_lists=True, swap=False):
    s, text, imgs = _world(rtw, knobs, swap)
    cam = _camera(rtw, cam_name)
    r, rays = _oracle(orc, text, imgs, swap, cam_name, cam, w, h, spp)
    off, rays_off, used_off, _ = _render(rtw, knobs, s, cam, w, h, spp, lists=False)
    assert used_off == 0
    _same(off, rays_off, r, rays, f"{cam_name} {w}x{h}x{spp}, lists off, vs the oracle")
    g, rays_g, used, over = _render(rtw, knobs, s, cam, w, h, spp)
    assert used == (1 if expect_lists else 0), f"{cam_name}: lists used = {used}"
    assert over == 0, f"{cam_name} {w}x{h}: {over} tiles on overflow"
    _same(g, rays_g, r, rays, f"{cam_name} {w}x{h}x{spp} vs the oracle")
    _same(g, rays_g, off, rays_off, f"{cam_name} {w}x{h}x{spp} vs lists off")
    return g


@pytest.mark.parametrize("cam_name", ["preset", "pinhole", "wide_lens", "inside", "down", "instant"])
def test_cameras(gpu, orc, knobs, cam_name):
    """The preset's camera, no lens, a wide beam (lens radius 0.5), a camera inside the cluster (boxes behind and around
    the lens), one looking straight down, and a shutter of [0.25, 0.25] (INSTANT_T1) against the first one's [0, 1]: 64x36x4."""
    _check(gpu, orc, knobs, cam_name, 64, 36, 4)


@pytest.mark.parametrize("w,h,spp", [(20, 20, 8), (13, 9, 8)])
def test_partial_tiles(gpu, orc, knobs, w, h, spp):
    """Frames whose last tile column and row lie partly outside the image."""
    _check(gpu, orc, knobs, "preset", w, h, spp)


def test_far_camera_keeps_lists_off(gpu, orc, knobs):
    """A camera inside the ground sphere, 1,200 units from the BVH: its lens is no near origin, so the host keeps the
    lists off, every start walks (the far-origin path), and the frame still matches."""
    _check(gpu, orc, knobs, "far", 48, 48, 2, expect_lists=False)


def test_tie_rule(gpu, orc, knobs):
    """Two coincident balls: the later one wins the tie, in the make step's fold as in the walk's, so swapping them
    changes the image, and each order matches the oracle."""
    a = _check(gpu, orc, knobs, "preset", 64, 36, 4)
    b = _check(gpu, orc, knobs, "preset", 64, 36, 4, swap=True)
    assert (a.view(np.uint32) != b.view(np.uint32)).any(), "swapping the coincident pair changed nothing"


def test_overflow_walks(gpu, orc, knobs):
    """RTW_TILE_LIST_CAP=1 under a camera so far out of focus that most tiles' beams cover several balls: those tiles
    overflow and their starts walk as before."""
    s, text, imgs = _world(gpu, knobs)
    cam = _camera(gpu, "blurred")
    w, h, spp = 64, 36, 4
    r, rays = _oracle(orc, text, imgs, False, "blurred", cam, w, h, spp)
    knobs.setenv("RTW_TILE_LIST_CAP", "1")
    g, rays_g, used, over = _render(gpu, knobs, s, cam, w, h, spp)
    assert used == 1 and over > gpu.n_tiles(w, h) // 2, (used, over, gpu.n_tiles(w, h))
    _same(g, rays_g, r, rays, "cap 1 vs the oracle")


def test_passes(gpu, orc, knobs):
    """A three-pass frame (RTW_PASS_LOG2=24: 4 slots of 64 x 65,536 ids per pass, 9 slots): the records are indexed by
    global tile id, whichever pass a tile falls in.  Against the one-pass frame with the lists off."""
    s, _, _ = _world(gpu, knobs)
    cam = _camera(gpu, "preset")
    w, h, spp = 20, 20, 65536
    off, rays_off, _, _ = _render(gpu, knobs, s, cam, w, h, spp, lists=False)
    knobs.setenv("RTW_PASS_LOG2", "24")
    g, rays_g, used, over = _render(gpu, knobs, s, cam, w, h, spp)
    assert used == 1 and over == 0
    _same(g, rays_g, off, rays_off, "three passes vs one pass, lists off")


def test_packed_and_strided_tiles(gpu, orc, knobs):
    """Packed tile renders for world sizes 1, 2 and 5, by id table and by stride: slots map to other tiles, the
    records stay with the tiles."""
    torch = pytest.importorskip("torch")
    rtw = gpu
    s, text, imgs = _world(rtw, knobs)
    cam = _camera(rtw, "preset")
    w, h, spp = 37, 21, 3
    r, rays = _oracle(orc, text, imgs, False, "preset", cam, w, h, spp)
    assert selected_kernel(s) == RING_KERNEL
    rt = rtw.Raytracer(s, cam, BG, w, h, spp, seed=SEED)
    nt = rtw.n_tiles(w, h)
    stream = torch.cuda.current_stream().cuda_stream
    for strided in (False, True):
        for world in (1, 2, 5):
            img = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
            n_rays = 0
            for rank in range(world):
                ids = torch.arange(rank, nt, world, dtype=torch.int32, device="cuda:0")
                packed = torch.zeros((len(ids), 64, 3), dtype=torch.float32, device="cuda:0")
                if strided:
                    st = rt.render_device_strided(packed.data_ptr(), 0, rank, world, len(ids), stream, want_stats=True)
                else:
                    st = rt.render_device(packed.data_ptr(), 0, ids.data_ptr(), len(ids), stream, want_stats=True)
                assert s.info(24) == 1 and s.info(25) == 0
                n_rays += st["rays"]
                rtw.unpack_tiles_device(w, h, ids.data_ptr(), len(ids), packed.data_ptr(), img.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            _same(img.cpu().numpy(), n_rays, r, rays, f"world {world} strided {strided}")


def test_count_build(gpu, orc, knobs):
    """The counting instantiation takes the same path: the plain build's frame and rays, and the make step's tests are
    counted as primitive tests while fewer nodes are visited than with the lists off."""
    torch = pytest.importorskip("torch")
    rtw = gpu
    s, text, imgs = _world(rtw, knobs)
    cam = _camera(rtw, "preset")
    w, h, spp = 64, 36, 4
    r, rays = _oracle(orc, text, imgs, False, "preset", cam, w, h, spp)
    assert selected_kernel(s) == RING_KERNEL
    stats = {}
    for lists in (True, False):
        if not lists:
            knobs.setenv("RTW_TILE_LISTS", "0")
        out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        st = rtw.Raytracer(s, cam, BG, w, h, spp, seed=SEED).render_device(
            out.data_ptr(), 0, 0, 0, torch.cuda.current_stream().cuda_stream, flags=rtw.FLAG_COUNT_TRAVERSAL,
            want_stats=True)
        assert s.info(24) == (1 if lists else 0)
        _same(out.cpu().numpy(), st["rays"], r, rays, f"count build, lists {lists}")
        stats[lists] = st
    assert 0 < stats[True]["node_visits"] < stats[False]["node_visits"], \
        (stats[True]["node_visits"], stats[False]["node_visits"])
    assert stats[True]["prim_tests"] > 0


def test_every_winner_is_in_its_tiles_list(gpu, knobs):
    """The superset property, directly: every camera ray of a 64x36x4 frame (rtw_camera_rays) whose closest hit
    (rtw_hit_rays, the walk) is a BVH primitive finds that primitive in its tile's record."""
    rtw = gpu
    s, _, _ = _world(rtw, knobs)
    w, h, spp = 64, 36, 4
    tiles_x = (w + 7) // 8
    for cam_name in ("preset", "wide_lens", "inside", "down"):
        cam = _camera(rtw, cam_name)
        lists, over, keys = rtw.diag_tile_lists(s, cam, w, h)
        assert over == 0 and len(keys) == 16
        prim_of_key = {int(k): p for p, k in enumerate(keys)}
        rays = s.camera_rays(cam, w, h, spp, SEED)
        hits = s.hit_rays(rays["origin"], rays["direction"], rays["time"], rays["stream"])
        p = np.arange(len(rays)) // spp  # p = (row * w + i) * spp + sample
        tile = (p // w // 8) * tiles_x + (p % w) // 8
        n_bvh_hits = 0
        for q in np.flatnonzero(hits["flags"] & 1):
            prim = prim_of_key.get(int(hits["key"][q]))
            if prim is None:  # the ground: always tested
                continue
            n_bvh_hits += 1
            assert prim in lists[tile[q]], \
                f"{cam_name}: path {q} (tile {tile[q]}) hits BVH primitive {prim}, not in its tile's list {lists[tile[q]]}"
        assert n_bvh_hits > 100, f"{cam_name}: only {n_bvh_hits} camera rays hit a BVH primitive"
