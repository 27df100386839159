"""Far-origin sphere hits (round 6).

The reference's f32 sphere test (spherical.rs:26-44) cancels in hb² - a·c: a ray whose origin is D away from a
sphere "hits" it up to ~sqrt(3u)·D outside its surface, and the flat list (hittable/mod.rs:57-69) finds every such
hit.  The GPU's BVH pads its sphere leaves for origins within D0 of the BVH and sends farther rays through the
far-origin walk (rtw_dev_trace.hpp trace_begin / trace_far).  These tests put the origin where the bound matters:
inside the r = 1000 ground sphere, under a field of small balls, bit for bit against the oracle with equal ray
counts; and the three random worlds of round 5's 3,000-seed run at 64x36x4 that the padded boxes alone missed.

The far camera runs under every kernel variant that carries the walk (the knob matrix below), over worlds whose
far leaves are every kind quad_radius (rtw_flatten.cpp) knows -- spheres, moving spheres, hollow shells, sphere-bounded
media -- and over the two kernels a far world reaches only by pick_kernel's rules (the generic kernel for a mesh world
with spheres in its BVH, the F_SMOKE kernel)."""
import numpy as np
import pytest

from test_gpu_fuzz import _random_world

pytestmark = pytest.mark.gpu

# rtw_device.hpp:147-179 (enum Feature and the kernel variants' feature sets), mirrored
F_SPHERE, F_MSPHERE, F_RECT, F_TRI, F_INST = 1 << 0, 1 << 1, 1 << 2, 1 << 3, 1 << 4
F_IMAGE, F_CHECKER, F_LAMBERT, F_METAL, F_DIEL, F_LIGHT = 1 << 6, 1 << 7, 1 << 9, 1 << 10, 1 << 11, 1 << 12
F_MEDIUM, F_ISO, F_TEXGEN = 1 << 13, 1 << 15, 1 << 17
F_SPHERES = F_SPHERE | F_MSPHERE | F_CHECKER | F_LAMBERT | F_METAL | F_DIEL | F_LIGHT
F_BOXES = F_RECT | F_INST | F_LAMBERT | F_METAL | F_DIEL | F_LIGHT
F_SMOKE = F_BOXES | F_MEDIUM | F_ISO
F_MESHES = F_SPHERE | F_RECT | F_TRI | F_INST | F_CHECKER | F_IMAGE | F_LAMBERT | F_LIGHT | F_TEXGEN
# rtw_dev_math.hpp: rows of the 32-bit LDS stack at 4 waves / SIMD and at 5-6 (STACK_LDS, STACK_LDS5)
STACK_LDS, STACK_LDS5 = 32, 24

BG = (0.7, 0.8, 1.0)
W = H = 48
SPP = 2
SEED = 11


def _ball_field(rtw, s, rng, n=14, moving=True, rotated=False):
    """jumpy-balls' shape in miniature: a checkered r = 1000 ground (always-tested) and an n x n grid of 0.2 balls
    (a BVH), some moving, optionally inside a YRotation + Translation."""
    ground = s.lambertian(s.checker(s.solid_rgb(0.2, 0.3, 0.1), s.solid_rgb(0.9, 0.9, 0.9), 10.0))
    s.sphere((0, -1000, 0), 1000, ground)
    mats = [s.lambertian_solid(tuple(rng.uniform(0.1, 0.9, 3))) for _ in range(3)]
    mats += [s.metal(tuple(rng.uniform(0.5, 1.0, 3)), 0.2), s.dielectric(1.5)]
    xs = np.arange(n, dtype=np.float32) - n / 2
    c = np.array([(a + 0.9 * rng.uniform(), 0.2, b + 0.9 * rng.uniform()) for a in xs for b in xs], np.float32)
    m = [int(rng.choice(mats)) for _ in range(len(c))]

    def add():
        k = len(c) // 2 if moving else len(c)
        s.spheres(c[:k], np.full(k, 0.2, np.float32), m[:k])
        if moving:
            c1 = c[k:] + np.array([0, 0.25, 0], np.float32) * rng.uniform(0, 1, (len(c) - k, 1)).astype(np.float32)
            s.moving_spheres(c[k:], np.zeros(len(c) - k), c1, np.ones(len(c) - k), np.full(len(c) - k, 0.2), m[k:])
    if rotated:
        with s.translate((0.3, 0.0, -0.2)):
            with s.rotate_y(17.0):
                add()
    else:
        add()


def _mesh_world(rtw, s, rng):
    """A mesh world with spheres in its BVH: the checkered ground, 64 Lambertian 0.2 balls and a tilted, tessellated
    quad of 72 triangles lying among them.  Every feature is one of F_MESHES, so but for the far rule
    (rtw_kernel.hip pick_kernel: `if (far) return pick5<F_ALL>(kn, need)`) this world would run the mesh kernels,
    which have no far path."""
    ground = s.lambertian(s.checker(s.solid_rgb(0.2, 0.3, 0.1), s.solid_rgb(0.9, 0.9, 0.9), 10.0))
    s.sphere((0, -1000, 0), 1000, ground)
    mats = [s.lambertian_solid(tuple(rng.uniform(0.1, 0.9, 3))) for _ in range(4)]
    xs = np.arange(8, dtype=np.float32) - 4
    c = np.array([(a + 0.9 * rng.uniform(), 0.2, b + 0.9 * rng.uniform()) for a in xs for b in xs], np.float32)
    s.spheres(c, np.full(len(c), 0.2, np.float32), [int(rng.choice(mats)) for _ in range(len(c))])
    g = 6  # g x g cells of two triangles over [-2, 2]^2, y rising from 0.05 to 0.45 along x
    p = np.linspace(-2.0, 2.0, g + 1, dtype=np.float32)

    def v(i, j):
        return (p[i], 0.05 + 0.1 * (p[i] + 2.0), p[j])
    tris = []
    for i in range(g):
        for j in range(g):
            tris += [v(i, j), v(i + 1, j), v(i + 1, j + 1), v(i, j), v(i + 1, j + 1), v(i, j + 1)]
    s.triangles(np.array(tris, np.float32).ravel(), mats[0])


def _shells_and_fog(rtw, s, rng):
    """The static ball field with ~10% of its balls hollow glass (a negative radius, spherical.rs:98-103) and three
    sphere-bounded ConstantMedium blobs among them: quad_radius' |r| of a negative radius and its medium branch as
    far leaves."""
    ground = s.lambertian(s.checker(s.solid_rgb(0.2, 0.3, 0.1), s.solid_rgb(0.9, 0.9, 0.9), 10.0))
    s.sphere((0, -1000, 0), 1000, ground)
    mats = [s.lambertian_solid(tuple(rng.uniform(0.1, 0.9, 3))) for _ in range(3)]
    mats += [s.metal(tuple(rng.uniform(0.5, 1.0, 3)), 0.2)]
    glass = s.dielectric(1.5)
    n = 14
    xs = np.arange(n, dtype=np.float32) - n / 2
    c = np.array([(a + 0.9 * rng.uniform(), 0.2, b + 0.9 * rng.uniform()) for a in xs for b in xs], np.float32)
    shell = rng.random(len(c)) < 0.1
    assert 10 <= shell.sum() <= 30
    m = np.array([int(rng.choice(mats)) for _ in range(len(c))])
    s.spheres(c[~shell], np.full(int((~shell).sum()), 0.2, np.float32), m[~shell])
    s.spheres(c[shell], np.full(int(shell.sum()), -0.2, np.float32), [glass] * int(shell.sum()))
    for (x, z, r, dens, rgb) in ((-2.3, 1.1, 0.3, 4.0, (0.9, 0.9, 0.9)), (1.4, -1.7, 0.45, 2.0, (0.1, 0.1, 0.1)),
                                 (3.1, 2.6, 0.6, 1.0, (0.8, 0.4, 0.2))):
        with s.constant_medium(dens, s.solid_rgb(*rgb)):
            s.sphere((x, r, z), r, mats[0])


def _smoke_world(rtw, s, rng):
    """A BVH of six Cuboids (36 rects, one of them rotated and translated) and 24 sphere-bounded ConstantMediums --
    no plain sphere anywhere, so the features stay within F_SMOKE -- hanging under a large light panel (one xz rect:
    always-tested, as the ground sphere is in the other worlds; an r = 1000 ground sphere would put F_SPHERE into
    the features).  The camera is 1,203 units below the panel, so every camera ray reaches the boxes and blobs as a
    far ray and takes the F_SMOKE kernel's copy of the far walk through rect and medium leaves."""
    white = s.lambertian_solid((0.73, 0.73, 0.73))
    red = s.lambertian_solid((0.65, 0.05, 0.05))
    steel = s.metal((0.8, 0.85, 0.9), 0.1)
    light = s.diffuse_light(s.solid_rgb(2.0, 2.0, 2.0))
    s.xz_rect(-1000.0, 1000.0, -1000.0, 1000.0, 3.0, light)
    for (x, z, m) in ((-5.0, -4.0, white), (1.5, 2.0, red), (3.5, -5.0, steel), (-3.0, 3.5, white), (-1.0, -2.0, red)):
        s.cuboid((x, 0.2, z), (x + 2.2, 1.6, z + 2.0), m)
    with s.translate((4.0, 0.3, 4.5)), s.rotate_y(25.0):
        s.cuboid((-1.0, 0.0, -1.0), (1.0, 1.5, 1.0), white)
    for k in range(24):
        r = float(rng.uniform(0.3, 0.6))
        x, z = rng.uniform(-6.0, 6.0, 2)
        with s.constant_medium(float(rng.uniform(0.5, 4.0)), s.solid_rgb(*rng.uniform(0.1, 0.9, 3))):
            s.sphere((float(x), float(rng.uniform(0.6, 2.0)), float(z)), r, white)


def _tall_field(rtw, s, rng):
    """The overflow test's own field: the static ball field's ground and 12 x 12 x 6 balls of 0.2 in a lattice 0.45
    apart, so that the boxes the far walk grows (by ~0.5 at 1,200 units) overlap their neighbours in every direction
    and the node4 tree is several levels deep."""
    ground = s.lambertian(s.checker(s.solid_rgb(0.2, 0.3, 0.1), s.solid_rgb(0.9, 0.9, 0.9), 10.0))
    s.sphere((0, -1000, 0), 1000, ground)
    mats = [s.lambertian_solid(tuple(rng.uniform(0.1, 0.9, 3))) for _ in range(3)]
    mats += [s.metal(tuple(rng.uniform(0.5, 1.0, 3)), 0.2), s.dielectric(1.5)]
    c = np.array([(0.45 * (a - 5.5) + 0.05 * rng.uniform(), 0.2 + 0.45 * k, 0.45 * (b - 5.5) + 0.05 * rng.uniform())
                  for a in range(12) for b in range(12) for k in range(6)], np.float32)
    s.spheres(c, np.full(len(c), 0.2, np.float32), [int(rng.choice(mats)) for _ in range(len(c))])


WORLDS = {
    "static": (1, lambda rtw, s, rng: _ball_field(rtw, s, rng, moving=False)),
    "moving": (2, lambda rtw, s, rng: _ball_field(rtw, s, rng, moving=True)),
    "rotated": (3, lambda rtw, s, rng: _ball_field(rtw, s, rng, moving=True, rotated=True)),
    "mesh": (4, _mesh_world),
    "shells_and_fog": (5, _shells_and_fog),
    "smoke": (6, _smoke_world),
    "tall": (7, _tall_field),
}
_REF = {}  # (world, max_depth) -> (scene text, oracle image, oracle rays): rendered once, shared, never written


def far_world(rtw, name):
    """-> (committed Scene, its text, its images, the far camera)."""
    seed, make = WORLDS[name]
    s = rtw.Scene()
    make(rtw, s, np.random.default_rng(seed))
    text, imgs = s.dump(), s.images()
    s.commit()
    cam = rtw.Camera.new((0.35, -1200.0, 0.15), (0.0, 0.2, 0.0), (1, 0, 0), 0.8, 1.0, 0.0, 1200.0)
    return s, text, imgs, cam


def far_reference(orc, name, text, imgs, cam, max_depth=50):
    """The oracle's frame of a far world, rendered once per (world, depth)."""
    key = (name, max_depth)
    if key not in _REF:
        r, rays = orc.OracleScene(text, imgs).render(orc.camera_from_fields(cam.as_dict()), BG, W, H, SPP, seed=SEED,
                                                     max_depth=max_depth)
        r.setflags(write=False)
        _REF[key] = (text, r, rays)
    t, r, rays = _REF[key]
    assert t == text, "the world's builder is not deterministic"
    return r, rays


def assert_far(s):
    """The far-origin bound is on, over a BVH, and D0 is far below the camera's 1,200 units: every camera ray is a
    far ray."""
    assert s.info(14) == 1 and s.info(3) > 0
    assert s.info(15) < 1000 * 1000


def assert_same(g, rays_g, r, rays):
    assert rays_g == rays, f"ray count {rays_g} vs oracle {rays}"
    bad = np.argwhere((g.view(np.uint32) != r.view(np.uint32)).any(axis=2))
    assert bad.size == 0, f"{len(bad)} mismatching pixels, first {bad[:4].tolist()}: " \
                          f"gpu {g[tuple(bad[0])]} oracle {r[tuple(bad[0])]}"


def _knob_preconditions(s, knob, sphere_world):
    """What pick_kernel (rtw_kernel.hip) checks before it returns the variant the knob is meant to select: a world
    outside these limits would quietly run another kernel."""
    n_nodes, need, need4, feat = s.info(3), s.info(8), s.info(11), s.info(9)
    assert (feat & ~F_SPHERES == 0) == sphere_world
    ks = dict(k.split("=") for k in knob.split(",")) if knob else {}
    if not sphere_world:  # pick5<F_ALL>, or the 4-wave F_ALL kernels
        assert need <= STACK_LDS5
        return
    if "RTW_STACK_LDS" in ks:  # path_kernel<4, SPILL, F_ALL>: the 4-entry column must be too short for the tree
        assert need > 4
    elif ks.get("RTW_OCC") == "4":  # path_kernel<STACK_LDS, no spill, 4, F_SPHERES>
        assert need <= STACK_LDS
    elif ks.get("RTW_OCC") == "5" or ks.get("RTW_LDS_NODES") == "0":
        # pick5<F_SPHERES or F_ALL> / path_kernel<STACK_LDS5, no spill, 6, F_SPHERES>: 32-bit stack, global node table
        assert need <= STACK_LDS5
    else:  # the LDS-node kernels: 16-bit codes (a half table exists only where they fit) and the table's capacity
        assert len(s.nodes_half()) > 0
        if ks.get("RTW_LDSN_WAVES") == "6":
            assert n_nodes <= 224 and need4 <= 24
        elif ks.get("RTW_LDSN_WAVES") == "7":
            assert n_nodes <= 160 and need4 <= 18
        else:  # 8 waves: 1024 lanes (the default, also under RTW_GENERIC alone: see below), 512 by knob / half nodes
            assert n_nodes <= 144 and need4 <= 16


# The kernel each knob selects, from pick_kernel, as rtw_scene_info 16-23 report it (KernelCfg: stack rows, HBM spill,
# waves / SIMD, feature set, workgroup size, node4s of the LDS node table, half nodes, 16-bit stack over global nodes)
F_ALL = ((1 << 16) - 1) | F_TEXGEN
SPHERE_KERNELS = {  # the sphere-only worlds (static, moving)
    "": (16, 0, 8, F_SPHERES, 1024, 144, 0, 0),                  # LDS nodes, 16-bit stack, 1024 lanes
    "RTW_LDS_NODES=0": (STACK_LDS5, 0, 6, F_SPHERES, 256, 0, 0, 0),  # global nodes, 32-bit stack
    # half nodes in LDS; the far walk reads the global f32 table, codes at +112
    "RTW_HALF_NODES=1": (16, 0, 8, F_SPHERES, 512, 144, 1, 0),
    "RTW_LDSN_WAVES=6": (24, 0, 6, F_SPHERES, 512, 224, 0, 0),
    "RTW_LDSN_WAVES=7": (18, 0, 7, F_SPHERES, 448, 160, 0, 0),
    "RTW_LDSN_BLK=512": (16, 0, 8, F_SPHERES, 512, 144, 0, 0),
    "RTW_OCC=5": (STACK_LDS5, 0, 5, F_SPHERES, 256, 0, 0, 0),    # pick5<F_SPHERES>
    "RTW_OCC=4": (STACK_LDS, 0, 4, F_SPHERES, 256, 0, 0, 0),
    # the default's kernel: pick_kernel reads RTW_GENERIC only on its default branch, which a sphere world (RTW_OCC's
    # default 6) leaves before; kept as the matrix lists it
    "RTW_GENERIC=1": (16, 0, 8, F_SPHERES, 1024, 144, 0, 0),
    "RTW_GENERIC=1,RTW_OCC=5": (STACK_LDS5, 0, 5, F_ALL, 256, 0, 0, 0),  # pick5<F_ALL>: the generic kernel, for real
    "RTW_STACK_LDS=4": (4, 1, 4, F_ALL, 256, 0, 0, 0),           # a 4-entry column, the far walk's overflow pass
}
ROTATED_KERNELS = {  # the rotated world (F_INST: not a sphere world)
    "": (STACK_LDS5, 0, 5, F_ALL, 256, 0, 0, 0),                 # pick5<F_ALL>
    "RTW_OCC=4": (STACK_LDS, 0, 4, F_ALL, 256, 0, 0, 0),
    "RTW_STACK_LDS=4": (4, 1, 4, F_ALL, 256, 0, 0, 0),
}


def selected_kernel(s):
    """rtw_scene_info 16-23: the path-kernel configuration the environment selects for s."""
    return tuple(s.info(16 + k) for k in range(8))


SPHERE_KNOBS = list(SPHERE_KERNELS)
FAR_MATRIX = [(v, k) for v in ("static", "moving") for k in SPHERE_KNOBS] + \
             [("rotated", k) for k in ROTATED_KERNELS]


@pytest.mark.parametrize("variant,knob", FAR_MATRIX)
def test_far_origin_camera_bit_exact(gpu, orc, knobs, variant, knob):
    """A camera inside the ground sphere, ~1,200 units below the ball field, looking up through it: every camera
    ray is a far-origin ray that reaches the field's grown box, and the ones that graze a ball within the sphere
    test's cancellation band hit it in the reference's list.  GPU == oracle bit for bit, equal ray counts, in every
    kernel variant that carries the far walk (the table above)."""
    rtw = gpu
    for kv in knob.split(",") if knob else ():
        knobs.setenv(*kv.split("="))
    s, text, imgs, cam = far_world(rtw, variant)
    assert_far(s)
    _knob_preconditions(s, knob, sphere_world=variant != "rotated")
    assert selected_kernel(s) == (ROTATED_KERNELS if variant == "rotated" else SPHERE_KERNELS)[knob]
    g, st = rtw.Raytracer(s, cam, BG, W, H, SPP, seed=SEED).render()
    r, rays = far_reference(orc, variant, text, imgs, cam)
    assert_same(g, st["rays"], r, rays)


def _count_render(rtw, s, cam, max_depth, flags):
    import torch
    out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    st = rtw.Raytracer(s, cam, BG, W, H, SPP, seed=SEED, max_depth=max_depth).render_device(
        out.data_ptr(), 0, 0, 0, torch.cuda.current_stream().cuda_stream, flags=flags, want_stats=True)
    return out.cpu().numpy(), st


def test_far_walk_overflow_pass_runs(gpu, orc, knobs):
    """trace_far's flat pass (a push beyond the lane's stack column marks `over`, then every BVH primitive is tested)
    shown to run, by the counting kernels.  At max_depth = 1 every segment is a camera ray from the far origin: the
    main walk never starts, and every primitive test comes from the always list or from trace_far.  RTW_STACK_LDS=4
    and RTW_GENERIC=1 with RTW_OCC=5 both run F_ALL kernels with a 32-bit stack (4 and 24 entries; RTW_GENERIC alone
    leaves a sphere world on its LDS-node kernel, see the table above), so the two walks are the same until a push
    overflows the 4 entries; the flat pass then adds n_bvh tests for that lane, more than the subtrees it replaces.
    Both frames equal the oracle's.
    Observed prim_tests (MI355X, 4,608 camera rays over 864 BVH balls): RTW_GENERIC=1,RTW_OCC=5 -> 208,677 (80,988
    node visits), RTW_STACK_LDS=4 -> 1,090,736 (55,770 node visits: the subtrees the overflow skipped)."""
    pytest.importorskip("torch")
    rtw = gpu
    tests = {}
    for knob in ("RTW_GENERIC=1,RTW_OCC=5", "RTW_STACK_LDS=4"):
        for kv in knob.split(","):
            knobs.setenv(*kv.split("="))
        s, text, imgs, cam = far_world(rtw, "tall")
        assert_far(s)
        assert s.info(9) & ~F_SPHERES == 0 and 4 < s.info(8) <= STACK_LDS5
        g, st = _count_render(rtw, s, cam, 1, rtw.FLAG_COUNT_TRAVERSAL)
        for kv in knob.split(","):
            knobs.delenv(kv.split("=")[0])
        r, rays = far_reference(orc, "tall", text, imgs, cam, max_depth=1)
        assert rays == W * H * SPP  # one segment per path
        assert_same(g, st["rays"], r, rays)
        assert st["boxes_tested"] == 0  # the main walk never ran: every node visit is trace_far's
        assert st["node_visits"] > 0
        tests[knob] = st["prim_tests"]
        print(f"far walk at max_depth 1, {knob}: prim_tests {st['prim_tests']}, node_visits {st['node_visits']}")
    assert tests["RTW_STACK_LDS=4"] > tests["RTW_GENERIC=1,RTW_OCC=5"], tests


@pytest.mark.parametrize("world", ["mesh", "shells_and_fog", "smoke"])
def test_far_origin_other_leaves_bit_exact(gpu, orc, world):
    """The far camera over worlds whose far leaves are not only plain spheres, each in the kernel pick_kernel sends
    it to: a mesh world with spheres in its BVH (the generic kernel, by the far rule), hollow shells and
    sphere-bounded media (the generic kernel), rects and sphere-bounded media alone (the F_SMOKE kernel)."""
    rtw = gpu
    s, text, imgs, cam = far_world(rtw, world)
    assert_far(s)
    feat = s.info(9)
    if world == "mesh":  # the mesh kernels' world but for `far`
        assert feat & F_TRI and feat & F_SPHERE and feat & ~F_MESHES == 0
    elif world == "shells_and_fog":
        assert feat & F_MEDIUM and feat & F_DIEL and feat & F_SPHERE
    else:  # pick5<F_SMOKE>, whose far_kernel_feat is true (F_MEDIUM)
        assert feat & ~F_SMOKE == 0 and feat & F_MEDIUM and feat & F_RECT and feat & ~F_BOXES != 0
    assert s.info(8) <= STACK_LDS5
    g, st = rtw.Raytracer(s, cam, BG, W, H, SPP, seed=SEED).render()
    r, rays = far_reference(orc, world, text, imgs, cam)
    assert_same(g, st["rays"], r, rays)


@pytest.mark.parametrize("seed", [863, 1981, 2503])
def test_far_origin_fuzz_regressions(gpu, orc, seed):
    """The random worlds whose 64x36x4 frames differed in round 5 (profiles/r05/r05fin_fuzz3000x4.log), each by one
    path bouncing inside the r = 1000 ground with a spurious small-sphere hit 1.9-2.8 r from its centre."""
    _random_world(gpu, orc, seed, 64, 36, 4)
