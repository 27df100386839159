"""Randomised worlds, GPU vs oracle, bit for bit.

Each seed builds a world from every kind the builder API has -- spheres (some hollow: negative radius), moving
spheres, rects of all three axes, cuboids under Translation / YRotation chains, triangles with and without vertex
normals and uvs, BvhNode groups (also nested inside wrappers), ConstantMedium with sphere and cuboid boundaries --
and every material / texture kind (Lambertian, Metal, Dielectric, DiffuseLight, Isotropic; solid, checker, Perlin
noise, an image, UV debug), then renders a small frame through whichever kernel variant the world selects (list
mode or a BVH, the generic or a specialised kernel).  The oracle's flat list (hittable/mod.rs:57-69) must agree
bit for bit, with the same ray count: the same property the preset scenes pin, over inputs nobody chose.
Round 5: 3,000 seeds at this frame were bit-exact, and at RTW_FUZZ_FRAME=64,36,4 three of 3,000 differed (863, 1981,
2503), each by one far-origin spurious sphere hit the BVH's padded boxes culled; round 6's far-origin walk (DESIGN.md
§2) matches them (tests/test_gpu_far.py keeps the three as regression tests)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP = (int(x) for x in os.environ.get("RTW_FUZZ_FRAME", "40,24,2").split(","))


def _build(rtw, s, rng):
    f = lambda *shape: rng.uniform(-1, 1, shape).astype(np.float32)
    texs = [s.solid_rgb(*rng.uniform(0.1, 0.95, 3)) for _ in range(3)]
    texs.append(s.checker(texs[0], texs[1], float(rng.uniform(1, 12))))
    texs.append(s.noise(float(rng.uniform(0.5, 5)), seed=int(rng.integers(1 << 30))))
    img = rng.integers(0, 256, (6, 9, 3), dtype=np.uint8)
    texs.append(s.image(img))
    texs.append(s.uv_debug())
    mats = [s.lambertian(int(rng.choice(texs))) for _ in range(4)]
    mats.append(s.metal(tuple(rng.uniform(0.3, 1.0, 3)), float(rng.uniform(0, 1))))
    mats.append(s.dielectric(float(rng.uniform(1.2, 2.0))))
    mats.append(s.diffuse_light(s.solid_rgb(*rng.uniform(1, 6, 3))))
    pick = lambda: int(rng.choice(mats))

    def spheres(n):
        c = f(n, 3) * 4
        r = rng.uniform(0.2, 1.0, n).astype(np.float32) * rng.choice([1, 1, 1, -1], n).astype(np.float32)
        s.spheres(c, r, [pick() for _ in range(n)])

    def moving(n):
        c0 = f(n, 3) * 4
        c1 = c0 + f(n, 3) * 0.5
        s.moving_spheres(c0, np.zeros(n), c1, np.ones(n), rng.uniform(0.2, 0.6, n), [pick() for _ in range(n)])

    def rects(n):
        a0 = f(n) * 4
        b0 = f(n) * 4
        s.rects(rng.integers(0, 3, n), a0, a0 + rng.uniform(0.5, 3, n), b0, b0 + rng.uniform(0.5, 3, n), f(n) * 5,
                [pick() for _ in range(n)])

    def tris(n):
        p = f(n, 1, 3) * 4 + f(n, 3, 3)
        nrm = f(n, 3, 3) if rng.uniform() < 0.5 else None
        uv = rng.uniform(0, 1, (n, 3, 2)).astype(np.float32) if rng.uniform() < 0.5 else None
        s.triangles(p.reshape(-1), pick(), normals=None if nrm is None else nrm.reshape(-1),
                    uvs=None if uv is None else uv.reshape(-1))

    spheres(int(rng.integers(1, 8)))
    rects(int(rng.integers(1, 6)))
    with s.translate(tuple(f(3) * 2)):
        with s.rotate_y(float(rng.uniform(-180, 180))):
            s.cuboid(tuple(f(3) - 1.5), tuple(f(3) + 1.5), pick())
    if rng.uniform() < 0.7:  # a BvhNode group, sometimes inside a wrapper
        with s.bvh():
            moving(int(rng.integers(2, 12)))
            tris(int(rng.integers(4, 40)))
            spheres(int(rng.integers(2, 10)))
    else:
        with s.rotate_y(float(rng.uniform(-90, 90))):
            with s.bvh():
                tris(int(rng.integers(4, 40)))
                moving(int(rng.integers(1, 6)))
    if rng.uniform() < 0.6:  # participating media (volumes.rs)
        with s.constant_medium(float(rng.uniform(0.05, 1.0)), int(rng.choice(texs[:3]))):
            if rng.uniform() < 0.5:
                s.sphere(tuple(f(3) * 3), float(rng.uniform(0.5, 1.5)), mats[0])
            else:
                with s.translate(tuple(f(3))):
                    s.cuboid(tuple(f(3) - 1), tuple(f(3) + 1), mats[0])
    s.sphere((0, -1000, 0), 1000, pick())  # the always-tested ground


@pytest.mark.parametrize("seed", range(int(os.environ.get("RTW_FUZZ_SEEDS", "24"))))
def test_random_world_bit_exact(gpu, orc, seed):
    _random_world(gpu, orc, seed, W, H, SPP)


def mixed_world(rtw, seed, W, H):
    """-> (the uncommitted scene of mixed world `seed`, its camera for a W x H frame, its background); imported by
    tests/test_ray_corpus.py too"""
    rng = np.random.default_rng(1000 + seed)
    s = rtw.Scene()
    _build(rtw, s, rng)
    eye = rng.uniform(-1, 1, 3) * np.array([8, 2, 8]) + np.array([0, 3, 0])
    cam = rtw.Camera.new(tuple(eye), tuple(rng.uniform(-1, 1, 3)), (0, 1, 0), float(rng.uniform(30, 70)), W / H,
                         float(rng.choice([0.0, 0.1])), float(np.linalg.norm(eye)))
    bg = tuple(rng.uniform(0, 0.8, 3))
    return s, cam, bg


def _random_world(rtw, orc, seed, W, H, SPP, max_depth=50):
    s, cam, bg = mixed_world(rtw, seed, W, H)
    text, imgs = s.dump(), s.images()
    s.commit()
    g, st = rtw.Raytracer(s, cam, bg, W, H, SPP, seed=seed, max_depth=max_depth).render()
    r, rays = orc.OracleScene(text, imgs).render(orc.camera_from_fields(cam.as_dict()), bg, W, H, SPP, seed=seed,
                                                max_depth=max_depth)
    assert st["rays"] == rays, f"ray count {st['rays']} vs oracle {rays}"
    bad = np.argwhere(g.view(np.uint32) != r.view(np.uint32))
    assert bad.size == 0, f"{len(bad)} mismatching components, first {bad[:4].tolist()}: " \
                          f"gpu {g[tuple(bad[0][:2])]} oracle {r[tuple(bad[0][:2])]}"


@pytest.mark.parametrize("max_depth", [50, 3])
def test_nan_throughput_world_bit_exact(gpu, orc, max_depth):
    """Round 6 (1,000 worlds at 96x54x8): world 329's UVDebug ground takes acos(-1.0000001) (spherical.rs:70-71), so
    some paths carry a NaN throughput; a Metal that absorbs, or the depth limit, ends them with black times the
    attenuations above (lib.rs:109-116): NaN, which the GPU once wrote as a constant 0."""
    _random_world(gpu, orc, 329, 96, 54, 8, max_depth)


@pytest.mark.parametrize("seed", range(int(os.environ.get("RTW_FUZZ_MESH_SEEDS", "6"))))
def test_random_mesh_bit_exact(gpu, orc, seed):
    """Random triangle soups of 1,500-6,000 triangles under one Translation, with a light rect and a checkered ground
    sphere: the mesh kernels (F_MESHES: triangle-only BVH leaves, half-precision nodes where built, the 16-bit-stack
    walk) on trees nobody tuned."""
    rtw = gpu
    s, cam, bg = mesh_world(rtw, seed)
    text, imgs = s.dump(), s.images()
    s.commit()
    g, st = rtw.Raytracer(s, cam, bg, W, H, SPP, seed=seed).render()
    r, rays = orc.OracleScene(text, imgs).render(orc.camera_from_fields(cam.as_dict()), bg, W, H, SPP, seed=seed)
    assert st["rays"] == rays
    bad = np.argwhere(g.view(np.uint32) != r.view(np.uint32))
    assert bad.size == 0, f"{len(bad)} mismatching components, first {bad[:4].tolist()}"
    assert s.info(3) > 0


def mesh_world(rtw, seed, max_triangles=None):
    """-> (the uncommitted scene of mesh world `seed`, its camera, its background); max_triangles caps the soup for
    tests/test_ray_corpus.py, whose oracle walks the flat list once per segment"""
    rng = np.random.default_rng(2000 + seed)
    n = int(rng.integers(1500, 6000))
    if max_triangles is not None:
        n = min(n, max_triangles)
    s = rtw.Scene()
    white = s.lambertian_solid((0.73, 0.73, 0.73))
    img = s.lambertian(s.image(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)))
    light = s.diffuse_light(s.solid_rgb(4, 4, 4))
    ground = s.lambertian(s.checker(s.solid_rgb(0.2, 0.3, 0.1), s.solid_rgb(0.9, 0.9, 0.9), 10.0))
    p = rng.normal(0, 1.5, (n, 1, 3)).astype(np.float32) + rng.uniform(-0.3, 0.3, (n, 3, 3)).astype(np.float32)
    uv = rng.uniform(0, 1, (n, 3, 2)).astype(np.float32)
    with s.translate(tuple(rng.uniform(-1, 1, 3))):
        s.triangles(p.reshape(-1), img if seed % 2 else white, uvs=uv.reshape(-1) if seed % 2 else None)
    s.xz_rect(-3, 3, -3, 3, 6, light)
    s.sphere((0, -1000, 0), 995, ground)
    cam = rtw.Camera.new((float(rng.uniform(-8, 8)), 2.0, 9.0), (0, 0, 0), (0, 1, 0), 45.0, W / H, 0.0, 9.0)
    bg = (0.1, 0.1, 0.15)
    return s, cam, bg
