"""The ring kernel's make retires the camera rays it resolves to a miss (path_kernel, K.ldsn_ring()).

A start whose tile list decides that it hits nothing is finished by the make itself: the lane writes the sample
(1 * bg) and the wave counts its one segment; off-image ids store nothing, and the remaining entries are packed against
the ring's top, each with its lane of origin.  A make may so yield fewer entries than the idle lanes want, or none (a
tile of sky), and the wave draws again.  None of this may change a bit: every case compares frame and ray count with
the ITERATIVE oracle and with the same build under RTW_TILE_LISTS=0 (no start decided, nothing retired), and asserts on
the oracle's frame alone the premise it is named for -- "all sky": every pixel is the in-order sum of spp backgrounds;
"mixed": some are and some are not.

World, cameras and helpers are tests/test_gpu_tile_lists.py's (the ground in the always-list, 16 BVH spheres)."""
import numpy as np
import pytest

import test_gpu_tile_lists as tl
from test_gpu_far import selected_kernel
from test_gpu_tile_lists import BG, RING_KERNEL, SEED, _oracle, _render, _same, _world

pytestmark = pytest.mark.gpu
f32 = np.float32


def _camera(rtw, name):
    new = rtw.Camera.new
    mine = {
        # straight up from the preset's eye: nothing but sky
        "sky": lambda: new((13, 2, 3), (13, 12, 3), (0, 0, -1), 20.0, 16 / 9, 0.1, 10.0, 0.0, 1.0),
        # rolled and raised: the ground fills the frame's top left corner only, so the bottom tile row and the right
        # tile column -- the partial ones of a frame that is no multiple of 8 -- are sky
        "tilted": lambda: new((13, 2, 3), (0, 3.5, 0), (-1, -1, 0.3), 20.0, 16 / 9, 0.1, 10.0, 0.0, 1.0),
        # level: the horizon runs through the middle of the frame
        "level": lambda: new((13, 2, 3), (0, 2, 0), (0, 1, 0), 20.0, 16 / 9, 0.1, 10.0, 0.0, 1.0),
    }
    return mine[name]() if name in mine else tl._camera(rtw, name)


def _sky_sum(spp):
    """spp backgrounds summed in order in f32: what reduce_kernel makes of an all-miss pixel"""
    t = np.zeros(3, f32)
    for _ in range(spp):
        t = t + np.array(BG, f32)
    return t


def _sky_mask(frame, spp):
    return (frame.view(np.uint32) == _sky_sum(spp).view(np.uint32)).all(axis=2)


def _premise(r, rays, premise, w, h, spp):
    sky = _sky_mask(r, spp)
    if premise == "all sky":
        assert sky.all() and rays == w * h * spp
    elif premise == "mixed":
        assert 0 < sky.sum() < sky.size
    elif premise == "no sky":
        assert not sky.any()
    elif premise == "sky edges":  # the partial tile row and column hold sky (and so off-image and retired lanes)
        assert w % 8 and h % 8 and sky[h - h % 8:].all() and sky[:, w - w % 8:].all() and not sky.all()
    else:
        raise AssertionError(premise)


def _check(rtw, orc, knobs, cam_name, w, h, spp, premise, set_knobs=()):
    """-> the frame; lists off and on (the latter under set_knobs) against the oracle and each other"""
    s, text, imgs = _world(rtw, knobs)
    cam = _camera(rtw, cam_name)
    r, rays = _oracle(orc, text, imgs, False, cam_name, cam, w, h, spp)
    _premise(r, rays, premise, w, h, spp)
    off, rays_off, used_off, _ = _render(rtw, knobs, s, cam, w, h, spp, lists=False)
    assert used_off == 0
    _same(off, rays_off, r, rays, f"{cam_name} {w}x{h}x{spp}, lists off, vs the oracle")
    for k, v in set_knobs:
        knobs.setenv(k, v)
    g, rays_g, used, over = _render(rtw, knobs, s, cam, w, h, spp)
    for k, _v in set_knobs:
        knobs.delenv(k)
    assert used == 1 and over == 0, (cam_name, used, over)
    _same(g, rays_g, r, rays, f"{cam_name} {w}x{h}x{spp} {set_knobs} vs the oracle")
    _same(g, rays_g, off, rays_off, f"{cam_name} {w}x{h}x{spp} {set_knobs} vs lists off")
    return g


def test_all_sky(gpu, orc, knobs):
    """Every path retires at the make, no ring entry is ever stored, and the render returns: no wave starves or spins.
    The frame is bg summed spp times in order and there is one ray per path."""
    w, h, spp = 64, 36, 4
    g = _check(gpu, orc, knobs, "sky", w, h, spp, "all sky")
    assert (g.view(np.uint32) == _sky_sum(spp).view(np.uint32)).all()


@pytest.mark.parametrize("cam_name,premise", [("preset", "mixed"), ("down", "no sky")])
def test_mixed_and_none(gpu, orc, knobs, cam_name, premise):
    """The preset camera (the horizon and the balls' silhouettes run through tiles: makes that retire some lanes) and
    the one looking down (no miss at all: nothing retires)."""
    _check(gpu, orc, knobs, cam_name, 64, 36, 4, premise)


@pytest.mark.parametrize("w,h,spp", [(13, 9, 8), (20, 20, 8)])
def test_partial_tiles_with_sky(gpu, orc, knobs, w, h, spp):
    """The partial last tile row and column are sky: off-image and retired lanes fall in the same make."""
    _check(gpu, orc, knobs, "tilted", w, h, spp, "sky edges")


@pytest.mark.parametrize("cam_name,premise", [("preset", "mixed"), ("sky", "all sky"), ("tilted", "mixed")])
@pytest.mark.parametrize("knob", [("RTW_BATCH", "64"), ("RTW_REGEN_MIN", "1"), ("RTW_REGEN_MIN", "64"),
                                  ("RTW_QUOTA16", "16")], ids=lambda k: f"{k[0]}={k[1]}")
def test_scheduling_extremes(gpu, orc, knobs, knob, cam_name, premise):
    """One make per pool refill, regeneration for a single idle lane and only for a whole idle wave (a short make
    leaves lanes idle: the wave must still draw again), and a walk that never hands control back early."""
    _check(gpu, orc, knobs, cam_name, 64, 36, 4, premise, set_knobs=(knob,))


@pytest.mark.parametrize("cam_name,premise", [("preset", "mixed"), ("sky", "all sky")])
@pytest.mark.parametrize("spp", [1, 3])
def test_sample_counts(gpu, orc, knobs, spp, cam_name, premise):
    """spp 1 and 3: passes whose last makes retire everything."""
    _check(gpu, orc, knobs, cam_name, 64, 36, spp, premise)


def test_overflow_misses_walk(gpu, orc, knobs):
    """RTW_TILE_LIST_CAP=1 under the out-of-focus camera: most tiles overflow, their starts are not decided, so their
    misses walk and end in the shading's miss branch; the rest retire.  The frame has both and still matches."""
    s, text, imgs = _world(gpu, knobs)
    cam = _camera(gpu, "blurred")
    w, h, spp = 64, 36, 4
    r, rays = _oracle(orc, text, imgs, False, "blurred", cam, w, h, spp)
    _premise(r, rays, "mixed", w, h, spp)
    knobs.setenv("RTW_TILE_LIST_CAP", "1")
    g, rays_g, used, over = _render(gpu, knobs, s, cam, w, h, spp)
    knobs.delenv("RTW_TILE_LIST_CAP")
    assert used == 1 and over > gpu.n_tiles(w, h) // 2, (used, over, gpu.n_tiles(w, h))
    _same(g, rays_g, r, rays, "cap 1 vs the oracle")
    off, rays_off, used_off, _ = _render(gpu, knobs, s, cam, w, h, spp, lists=False)
    assert used_off == 0
    _same(g, rays_g, off, rays_off, "cap 1 vs lists off")


def test_packed_and_strided_tiles_with_sky(gpu, orc, knobs):
    """Packed tile renders for world sizes 2 and 5, by id table and by stride, under the level camera (half the frame
    is sky): a retired path's sample slot follows its slot in the subset, not its tile."""
    torch = pytest.importorskip("torch")
    rtw = gpu
    s, text, imgs = _world(rtw, knobs)
    cam = _camera(rtw, "level")
    w, h, spp = 37, 21, 3
    r, rays = _oracle(orc, text, imgs, False, "level", cam, w, h, spp)
    sky = _sky_mask(r, spp)
    assert 0.3 < sky.mean() < 0.7, sky.mean()
    assert selected_kernel(s) == RING_KERNEL
    rt = rtw.Raytracer(s, cam, BG, w, h, spp, seed=SEED)
    nt = rtw.n_tiles(w, h)
    stream = torch.cuda.current_stream().cuda_stream
    for strided in (False, True):
        for world in (2, 5):
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


@pytest.mark.parametrize("cam_name,premise", [("preset", "mixed"), ("sky", "all sky")])
def test_count_build(gpu, orc, knobs, cam_name, premise):
    """The counting instantiation retires the same paths: the oracle's frame and rays, and the make's tests counted."""
    torch = pytest.importorskip("torch")
    rtw = gpu
    s, text, imgs = _world(rtw, knobs)
    cam = _camera(rtw, cam_name)
    w, h, spp = 64, 36, 4
    r, rays = _oracle(orc, text, imgs, False, cam_name, cam, w, h, spp)
    _premise(r, rays, premise, w, h, spp)
    assert selected_kernel(s) == RING_KERNEL
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    st = rtw.Raytracer(s, cam, BG, w, h, spp, seed=SEED).render_device(
        out.data_ptr(), 0, 0, 0, torch.cuda.current_stream().cuda_stream, flags=rtw.FLAG_COUNT_TRAVERSAL,
        want_stats=True)
    assert s.info(24) == 1
    _same(out.cpu().numpy(), st["rays"], r, rays, f"count build, {cam_name}")
    assert st["prim_tests"] > 0


@pytest.mark.parametrize("cam_name", ["preset", "sky"])
def test_progressive_ranges(gpu, knobs, cam_name):
    """rtw_render_samples_device over [0, 3) and [3, 8) against [0, 8) in one call: sums, sums of squares and rays.
    The retired paths write the same sample slots as the paths that walk."""
    torch = pytest.importorskip("torch")
    rtw = gpu
    s, _text, _imgs = _world(rtw, knobs)
    cam = _camera(rtw, cam_name)
    w, h, spp = 64, 36, 8
    assert selected_kernel(s) == RING_KERNEL
    rt = rtw.Raytracer(s, cam, BG, w, h, spp, seed=SEED)
    stream = torch.cuda.current_stream().cuda_stream
    res = []
    for ranges in ([(0, 3), (3, 5)], [(0, 8)]):
        d_sum = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        d_sq = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        n_rays = 0
        for first, n in ranges:
            st = rt.render_samples_device(d_sum.data_ptr(), d_sq.data_ptr(), first, n, device=0, stream_ptr=stream,
                                          want_stats=True)
            assert s.info(24) == 1
            n_rays += st["rays"]
        res.append((d_sum.cpu().numpy(), d_sq.cpu().numpy(), n_rays))
    (a, a_sq, rays_a), (b, b_sq, rays_b) = res
    _same(a, rays_a, b, rays_b, f"{cam_name}: sums over two ranges vs one")
    _same(a_sq, rays_a, b_sq, rays_b, f"{cam_name}: sums of squares over two ranges vs one")
    if cam_name == "sky":
        assert rays_a == w * h * spp and (a.view(np.uint32) == _sky_sum(spp).view(np.uint32)).all()
