"""The start ring of the 1024-lane LDS-node sphere kernel (rtw_path_kernel.hpp path_kernel SRING,
KernelCfg::ldsn_ring).

Each wave of that kernel makes 64 path starts at a time from 64 consecutive ids of its pool -- start_make's half of a
start, 7 words per entry -- and a regenerating lane finishes the entry it takes (start_take).  A path's start is a
function of its id alone, so the frame and the ray count must be those of a kernel without the ring.  The reference
here is the same frame under RTW_LDS_NODES=0: the global-node sphere kernel, whose every lane runs start_path for
its own id.  Frames are compared bit for bit (uint32 view), ray counts for equality.

The frames are the smallest at which the ring can go wrong: ragged ones (off-image ids inside a ring), one tile with
15 live ids of 64 (one ring, then the pool is dry), exactly one ring, passes, packed and strided tiles, batches of one
ring, both dispenser layouts, both ends of regen_min, and the counting build."""
import numpy as np
import pytest

from test_gpu_far import F_SPHERES, STACK_LDS5, _ball_field, selected_kernel

pytestmark = pytest.mark.gpu

BG = (0.7, 0.8, 1.0)
SEED = 5
RING_KERNEL = (16, 0, 8, F_SPHERES, 1024, 144, 0, 0)        # spheres_ldsn1024x144: the kernel under test
PLAIN_KERNEL = (STACK_LDS5, 0, 6, F_SPHERES, 256, 0, 0, 0)  # RTW_LDS_NODES=0: global nodes, per-lane starts
RAGGED = (37, 21, 3)  # 5 x 3 tiles, the last column and row partly outside the image

_WORLD = []
_REF = {}  # (w, h, spp) -> (frame, rays) of the plain kernel: rendered once, shared, never written


def _world(rtw):
    """The miniature jumpy-balls of test_gpu_far (half its balls moving) under a camera with a lens and a shutter, so
    that every word of a ring entry and start_take's time draw matter."""
    if not _WORLD:
        s = rtw.Scene()
        _ball_field(rtw, s, np.random.default_rng(2), moving=True)
        s.commit(device=0)
        cam = rtw.Camera.new((6.0, 2.0, 4.0), (0.0, 0.3, 0.0), (0, 1, 0), 30.0, 37 / 21, 0.1, 7.0, 0.0, 1.0)
        _WORLD.append((s, cam))
    return _WORLD[0]


def _reference(rtw, knobs, w, h, spp):
    s, cam = _world(rtw)
    if (w, h, spp) not in _REF:
        knobs.setenv("RTW_LDS_NODES", "0")
        assert selected_kernel(s) == PLAIN_KERNEL
        r, st = rtw.Raytracer(s, cam, BG, w, h, spp, seed=SEED).render()
        knobs.delenv("RTW_LDS_NODES")
        r.setflags(write=False)
        _REF[(w, h, spp)] = (r, st["rays"])
    return _REF[(w, h, spp)]


def _assert_same(g, rays_g, r, rays, what=""):
    assert rays_g == rays, f"{what}: ray count {rays_g} vs the plain kernel's {rays}"
    bad = np.argwhere((g.view(np.uint32) != r.view(np.uint32)).any(axis=2))
    assert bad.size == 0, f"{what}: {len(bad)} mismatching pixels, first {bad[:4].tolist()}: " \
                          f"ring {g[tuple(bad[0])]} plain {r[tuple(bad[0])]}"


def _check(rtw, knobs, w, h, spp, env=()):
    s, cam = _world(rtw)
    r, rays = _reference(rtw, knobs, w, h, spp)
    for k, v in env:
        knobs.setenv(k, v)
    assert selected_kernel(s) == RING_KERNEL  # otherwise the frame says nothing about the ring
    g, st = rtw.Raytracer(s, cam, BG, w, h, spp, seed=SEED).render()
    _assert_same(g, st["rays"], r, rays, f"{w}x{h}x{spp} {dict(env)}")


@pytest.mark.parametrize("w,h,spp", [RAGGED, (5, 3, 1), (8, 8, 1)])
def test_ring_frames(gpu, knobs, w, h, spp):
    """The ragged frame; one tile with 15 live ids of 64 (the ring is made once, with 49 off-image entries, and the
    pool then runs dry); exactly one ring with every entry live."""
    _check(gpu, knobs, w, h, spp)


@pytest.mark.parametrize("knob", ["RTW_BATCH=64", "RTW_BATCH=100", "RTW_BATCH=1024", "RTW_REGEN_MIN=1",
                                  "RTW_REGEN_MIN=64", "RTW_QUOTA16=1"])
def test_ring_knobs(gpu, knobs, knob):
    """Batches of exactly one ring (64, and 100 rounded down to it), the full-frame batch of 1024 with its single
    dispenser, regeneration at the first idle lane and only when the whole wave is idle, and the smallest traversal
    quota (the most suspended walks between regenerations): the ragged frame each time."""
    _check(gpu, knobs, *RAGGED, env=[tuple(knob.split("="))])


def test_ring_sharded_dispensers(gpu, knobs):
    """A small frame's batch is cut below 1024 by the host (to 128), so the 8 dispensers are active, as with
    configs[0]: 160x90x8 is 900 batches of 128 over them, and most of the grid's waves find every dispenser dry."""
    _check(gpu, knobs, 160, 90, 8)


def test_ring_passes(gpu, knobs):
    """A frame in three passes (RTW_PASS_LOG2=24: 4 tile slots of 64 x 65,536 ids each per pass, 9 slots): the pool
    and the ring restart at every pass.  The reference is the plain kernel's one-pass frame."""
    _check(gpu, knobs, 20, 20, 65536, env=[("RTW_PASS_LOG2", "24")])


def test_ring_packed_and_strided_tiles(gpu, knobs):
    """The ragged frame as packed tile renders for world sizes 1, 2 and 5, by id table and by stride: short passes
    whose slots map to other tiles, against the one-pass full frame."""
    torch = pytest.importorskip("torch")
    rtw = gpu
    s, cam = _world(rtw)
    w, h, spp = RAGGED
    r, rays = _reference(rtw, knobs, w, h, spp)
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
                n_rays += st["rays"]
                rtw.unpack_tiles_device(w, h, ids.data_ptr(), len(ids), packed.data_ptr(), img.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            _assert_same(img.cpu().numpy(), n_rays, r, rays, f"world {world} strided {strided}")


def test_ring_count_build(gpu, knobs):
    """The counting instantiation (FLAG_COUNT_TRAVERSAL) of the ring kernel: the same rays and frame as the plain
    build, and the time it books to path starts lies within regeneration's."""
    torch = pytest.importorskip("torch")
    rtw = gpu
    s, cam = _world(rtw)
    w, h, spp = RAGGED
    r, rays = _reference(rtw, knobs, w, h, spp)
    assert selected_kernel(s) == RING_KERNEL
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    st = rtw.Raytracer(s, cam, BG, w, h, spp, seed=SEED).render_device(
        out.data_ptr(), 0, 0, 0, torch.cuda.current_stream().cuda_stream, flags=rtw.FLAG_COUNT_TRAVERSAL,
        want_stats=True)
    _assert_same(out.cpu().numpy(), st["rays"], r, rays, "count build")
    share = st["phase_share"]
    assert st["node_visits"] > 0 and share["regen"] > 0
    assert 0 < share["path_start"] <= share["regen"], share
