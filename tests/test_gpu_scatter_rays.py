"""Scatter and camera-ray queries on the GPU (rtw_scatter_rays*, rtw_camera_rays*: Material::scatter + emitted,
material.rs:23-26 and light_source.rs:17-24; Camera::get_ray, camera.rs:66-74).

Every comparison is bit for bit, on uint32 views: the camera rays against the oracle's get_ray on the oracle's draws,
the scatter records against oracle_scatter on the oracle's draws, and a wavefront integrator written here from the three
queries (camera_rays -> (hit_rays -> scatter_rays)*) against the oracle's render: same image, same ray count.

The block of scatter records (4,099 per material, shuffled, with misses between) and the oracle's answers for it are
made once and shared by the tests that need them."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32
_F = C.POINTER(C.c_float)
_U32 = C.POINTER(C.c_uint32)
N_PER = 4099
N_MISS = 1000
N_DRAWS = 96
BG = (0.25, 0.5, 0.75)
LIGHT = (4.0, 3.0, 2.0)
# slot -> (oracle_scatter kind, albedo, fuzz / ir); slot 4 is the DiffuseLight
MATS = [(0, (0.8, 0.3, 0.1), 0.0), (1, (0.9, 0.8, 0.7), 1.0), (1, (0.6, 0.7, 0.8), 0.3), (2, (1.0, 1.0, 1.0), 1.5)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_records(got, want, what):
    a = np.frombuffer(np.ascontiguousarray(got).tobytes(), np.uint32).reshape(len(got), -1)
    b = np.frombuffer(np.ascontiguousarray(want).tobytes(), np.uint32).reshape(len(want), -1)
    assert a.shape == b.shape, what
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} records differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


# ---------------------------------------------------------------- 1. camera rays
def _oracle_camera_rays(orc, ocam, w, h, spp, seed):
    """start_path per path, in the output's order p = ((h-1-j)*w + i)*spp + s (lib.rs:84-86, camera.rs:66-74): the
    oracle's path state through its generator, u and v in numpy float32, oracle_get_ray on the remaining draws."""
    L = orc.lib()
    rays = np.zeros(w * h * spp, [("origin", f32, 3), ("direction", f32, 3), ("time", f32), ("reserved", np.uint32),
                                  ("stream", np.uint64)])
    draws, out, used, after = np.zeros(64, np.uint32), np.zeros(7, f32), C.c_uint32(), C.c_uint64()
    dp = draws.ctypes.data_as(_U32)
    for j in range(h):
        for i in range(w):
            for s in range(spp):
                state = L.oracle_path_state(seed, j, i, s)
                L.oracle_rng_stream(state, 64, dp, C.byref(after))
                u = f32(f32(i) + f32(L.oracle_u32_to_f32(int(draws[0])))) / f32(w - 1)
                v = f32(f32(j) + f32(L.oracle_u32_to_f32(int(draws[1])))) / f32(h - 1)
                L.oracle_get_ray(C.byref(ocam), u, v, C.cast(draws.ctypes.data + 8, _U32), 62, out.ctypes.data_as(_F),
                                 C.byref(used))
                assert used.value <= 60
                L.oracle_rng_stream(state, 2 + used.value, dp, C.byref(after))
                p = ((h - 1 - j) * w + i) * spp + s
                rays[p] = (out[0:3], out[3:6], out[6], 0, after.value)
    return rays


@pytest.mark.parametrize("name,aspect,aperture", [("jumpy-balls", 16 / 9, 0.1), ("cornell-box", 1.0, 0.0)])
def test_camera_rays_match_the_oracle(gpu, orc, name, aspect, aperture):
    w, h, spp, seed = 13, 7, 3, 11  # 273 rays: a partial last wave
    s = gpu.Scene()
    cam, _bg = s.preset(name, aspect, seed=3)
    assert (cam.c.lens_radius == 0.0) == (aperture == 0.0) and cam.c.time0 < cam.c.time1
    if name == "jumpy-balls":
        assert (cam.c.time0, cam.c.time1) == (0.0, 1.0)
    s.commit(device=0)
    want = _oracle_camera_rays(orc, orc.camera_from_fields(cam.as_dict()), w, h, spp, seed)
    assert (want["stream"] != 0).all() and len(np.unique(want["stream"])) == len(want)
    got = s.camera_rays(cam, w, h, spp, seed, device=0)
    assert got.dtype == gpu.RAY_DTYPE and len(got) == 273
    _same_records(got, want, f"{name} camera rays")
    part = s.camera_rays(cam, w, h, spp, seed, first=100, n=65, device=0)
    _same_records(part, got[100:165], "paths [100, 165)")
    for n in (1, 63, 64):
        _same_records(s.camera_rays(cam, w, h, spp, seed, first=273 - n, n=n, device=0), got[273 - n:], f"last {n}")


# ---------------------------------------------------------------- 2. scatter records
@pytest.fixture(scope="module")
def mat_scene(gpu):
    """One sphere per material: Lambertian(solid), Metal fuzz 1.0, Metal fuzz 0.3, Dielectric 1.5, DiffuseLight."""
    s = gpu.Scene()
    ids = [s.lambertian_solid(MATS[0][1]), s.metal(MATS[1][1], MATS[1][2]), s.metal(MATS[2][1], MATS[2][2]),
           s.dielectric(MATS[3][2]), s.diffuse_light(s.solid_rgb(*LIGHT))]
    for k, m in enumerate(ids):
        s.sphere((3.0 * k, 0.0, 0.0), 1.0, m)
    s.commit(device=0)
    return s, ids


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _block(rtw, orc, ids):
    """-> (rays, hits, want_rays, want_scatter, slot per record (-1 = miss), draws used per record), shuffled."""
    rng = np.random.default_rng(7)
    n = 5 * N_PER + N_MISS
    slot = np.concatenate([np.repeat(np.arange(5), N_PER), np.full(N_MISS, -1)])
    normal = _unit(rng.normal(size=(n, 3)))
    d = rng.normal(size=(n, 3))
    graze = rng.random(n) < 0.25
    tang = rng.normal(size=(n, 3))
    tang = _unit(tang - normal * (tang * normal).sum(axis=1, keepdims=True))
    d[graze] = (tang + normal * rng.uniform(-0.05, 0.05, (n, 1)))[graze]
    d = (d * rng.uniform(0.1, 5.0, (n, 1))).astype(f32)
    normal = normal.astype(f32)
    normal[(d.astype(np.float64) * normal.astype(np.float64)).sum(axis=1) > 0] *= f32(-1)  # opposes the direction
    rays = rtw.make_rays(rng.uniform(-5, 5, (n, 3)), d, rng.random(n).astype(f32),
                         rng.integers(1, 1 << 63, n, dtype=np.uint64))
    hits = np.zeros(n, rtw.HIT_DTYPE)
    hits["p"] = rng.uniform(-5, 5, (n, 3))
    hits["normal"] = normal
    hits["t"] = rng.uniform(0.01, 9.0, n)
    hits["u"], hits["v"] = rng.random(n), rng.random(n)
    hits["key"] = np.maximum(slot, 0)
    hits["material"] = np.asarray(ids, np.uint32)[np.maximum(slot, 0)]
    front = np.ones(n, bool)
    front[slot == 3] = np.arange(N_PER) % 2 == 0  # the dielectric's records alternate FRONT_FACE
    hits["flags"] = rtw.HIT_HIT | np.where(front, rtw.HIT_FRONT_FACE, 0)
    miss = slot < 0
    hits[miss] = np.zeros(int(miss.sum()), rtw.HIT_DTYPE)
    hits["t"][miss] = np.inf
    perm = rng.permutation(n)
    rays, hits, slot, front = rays[perm], hits[perm], slot[perm], front[perm]
    # the oracle's answers
    L = orc.lib()
    want_r, want_s = rays.copy(), np.zeros(n, rtw.SCATTER_DTYPE)
    used_all = np.zeros(n, np.int64)
    draws, out, used, after = np.zeros(N_DRAWS, np.uint32), np.zeros(6, f32), C.c_uint32(), C.c_uint64()
    dp = draws.ctypes.data_as(_U32)
    for k in range(n):
        if slot[k] < 0:
            want_s[k] = ((0, 0, 0), BG, rtw.SCATTER_MISS, 0)  # the ray copied through
            continue
        want_r["origin"][k] = hits["p"][k]
        if slot[k] == 4:  # the light: emits, no draws
            want_s[k] = ((0, 0, 0), LIGHT, 0, 0)
            continue
        kind, albedo, param = MATS[slot[k]]
        state = int(rays["stream"][k])
        L.oracle_rng_stream(state, N_DRAWS, dp, C.byref(after))
        ray7 = np.array([*rays["origin"][k], *rays["direction"][k], rays["time"][k]], f32)
        rec7 = np.array([*hits["p"][k], *hits["normal"][k], 1.0 if front[k] else 0.0], f32)
        ok = L.oracle_scatter(kind, orc.fp(orc.f32([*albedo, param])), orc.fp(ray7), orc.fp(rec7), dp, N_DRAWS,
                              out.ctypes.data_as(_F), C.byref(used))
        L.oracle_rng_stream(state, used.value, dp, C.byref(after))
        used_all[k] = used.value
        want_r["direction"][k] = out[0:3]
        want_r["stream"][k] = after.value if used.value else state
        want_s[k] = (out[3:6] if ok else (0, 0, 0), (0, 0, 0), rtw.SCATTER_SCATTERED if ok else 0, 0)
    for a in (rays, hits, want_r, want_s, slot, used_all):
        a.setflags(write=False)
    return rays, hits, want_r, want_s, slot, used_all


def test_the_block_covers_the_branches(gpu, orc, mat_scene):
    """From the oracle's answers alone."""
    _s, ids = mat_scene
    _rays, _hits, _wr, ws, slot, used = _block(gpu, orc, tuple(ids))
    scattered = (ws["flags"] & gpu.SCATTER_SCATTERED) != 0
    fuzz1 = slot == 1
    assert (fuzz1 & ~scattered).sum() >= 500 and (fuzz1 & scattered).sum() >= 2000, \
        ((fuzz1 & ~scattered).sum(), (fuzz1 & scattered).sum())
    diel = slot == 3
    assert (diel & (used == 0)).sum() >= 1000 and (diel & (used == 1)).sum() >= 1000, \
        ((diel & (used == 0)).sum(), (diel & (used == 1)).sum())
    assert set(np.unique(used[diel])) == {0, 1} and scattered[diel].all()
    assert used[slot == 0].max() >= 8 * 3, used[slot == 0].max()  # some Lambertian record with >= 8 rejection trips
    assert (used % 3 == 0)[(slot >= 0) & (slot <= 2)].all()
    assert used.max() < N_DRAWS, "no record may run out of the draws handed to the oracle"


def test_scatter_records_match_the_oracle(gpu, orc, mat_scene):
    s, ids = mat_scene
    rays, hits, want_r, want_s, slot, _used = _block(gpu, orc, tuple(ids))
    out, sc = s.scatter_rays(rays, hits, BG, device=0)
    for name, m in (("miss", slot < 0), ("lambertian", slot == 0), ("metal fuzz 1", slot == 1),
                    ("metal fuzz 0.3", slot == 2), ("dielectric", slot == 3), ("light", slot == 4)):
        assert m.sum() >= N_MISS
        _same_records(sc[m], want_s[m], f"{name}: scatter records")
        if name == "light":  # no ray to follow: the stream unchanged, nothing drawn
            assert (out["stream"][m] == rays["stream"][m]).all() and (out["time"][m] == rays["time"][m]).all()
        else:  # direction, stream after the draws, origin = p, time kept (a miss: the ray unchanged)
            _same_records(out[m], want_r[m], f"{name}: out rays")
    assert (_bits(sc["emitted"][slot < 0]) == _bits(np.asarray(BG, f32))).all()
    assert (_bits(sc["emitted"][slot == 4]) == _bits(np.asarray(LIGHT, f32))).all()
    assert (sc["emitted"][(slot >= 0) & (slot < 4)] == 0).all() and (sc["reserved"] == 0).all()


# ---------------------------------------------------------------- 3. bad records
def _device_scatter(gpu, s, rays, hits, bg, in_place=False, stream=None):
    import torch
    dev = torch.device("cuda:0")
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).to(dev)
    d_hits = torch.from_numpy(np.ascontiguousarray(hits).view(np.uint8).reshape(-1).copy()).to(dev)
    d_out = d_rays if in_place else torch.zeros(n * 40, dtype=torch.uint8, device=dev)
    d_sc = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    s.scatter_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), bg, d_out.data_ptr(), d_sc.data_ptr(), n, 0,
                          stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize(dev)
    return (np.frombuffer(d_out.cpu().numpy().tobytes(), gpu.RAY_DTYPE),
            np.frombuffer(d_sc.cpu().numpy().tobytes(), gpu.SCATTER_DTYPE))


def test_bad_records_leave_their_neighbours_alone(gpu, orc, mat_scene):
    """(scatter_kernel mends the caller's generator state with xoro_seed before anything can draw from it, so the zero
    stream word below cannot reach a rejection loop.)"""
    s, ids = mat_scene
    rays, hits, want_r, want_s, _slot, _used = _block(gpu, orc, tuple(ids))
    n = 130
    rays, hits = rays[:n].copy(), hits[:n].copy()
    n_mats = s.info(1)
    assert n_mats == len(ids)
    good_out, good_sc = _device_scatter(gpu, s, rays, hits, BG)
    _same_records(good_sc, want_s[:n], "device form")
    _same_records(good_out[_slot[:n] != 4], want_r[:n][_slot[:n] != 4], "device form: out rays")
    bad = np.array([5, 63, 64, 129])
    hits["flags"][bad[:2]] = gpu.HIT_HIT | gpu.HIT_FRONT_FACE
    hits["material"][bad[0]] = n_mats
    hits["material"][bad[1]] = 0xFFFFFFFF
    hits["flags"][bad[2]] = gpu.HIT_BAD_RAY
    rays["stream"][bad[3]] = 0
    out, sc = _device_scatter(gpu, s, rays, hits, BG)
    assert (sc["flags"][bad] == gpu.SCATTER_BAD).all()
    assert (_bits(sc["attenuation"][bad]) == 0).all() and (_bits(sc["emitted"][bad]) == 0).all()
    assert (np.frombuffer(out[bad].tobytes(), np.uint32) == 0).all()
    keep = np.ones(n, bool)
    keep[bad] = False
    _same_records(sc[keep], good_sc[keep], "scatter records beside the bad ones")
    _same_records(out[keep], good_out[keep], "out rays beside the bad ones")


# ---------------------------------------------------------------- 4. the caller's integrator
def _integrate(gpu, s, cam, bg, w, h, spp, seed, max_depth):
    """sample_ray (lib.rs:97-117) as a wavefront loop over the three host queries -> (image sums [h, w, 3], rays)."""
    rays = s.camera_rays(cam, w, h, spp, seed, device=0)
    n = len(rays)
    T, L, path, nrays = np.ones((n, 3), f32), np.zeros((n, 3), f32), np.arange(n), 0
    zero = f32(0.0)
    with np.errstate(all="ignore"):
        for depth in range(max_depth, 0, -1):
            if len(rays) == 0:
                break
            hits = s.hit_rays(rays["origin"], rays["direction"], rays["time"], rays["stream"], device=0)
            nrays += len(rays)
            out, sc = s.scatter_rays(rays, hits, bg, device=0)
            assert not (sc["flags"] & gpu.SCATTER_BAD).any()
            alive = (sc["flags"] & gpu.SCATTER_SCATTERED) != 0
            L[path[~alive]] = T[path[~alive]] * sc["emitted"][~alive]
            T[path[alive]] = T[path[alive]] * sc["attenuation"][alive]
            path, rays = path[alive], out[alive]
            if depth == 1:
                L[path] = T[path] * zero  # lib.rs:98-100: black, times the attenuations above it
        pixel = np.zeros((h * w, 3), f32)
        Ls = L.reshape(h * w, spp, 3)
        for k in range(spp):  # float32 throughout, in sample order, as reduce_kernel
            pixel = pixel + Ls[:, k]
    assert T.dtype == f32 and L.dtype == f32 and pixel.dtype == f32
    return pixel.reshape(h, w, 3), nrays


@pytest.mark.parametrize("name,aspect,w,h,spp,max_depth", [
    ("jumpy-balls", 16 / 9, 48, 27, 2, 50),
    ("cornell-box", 1.0, 24, 24, 4, 50),
    ("cornell-box", 1.0, 24, 24, 4, 3),  # depth exhaustion
    ("smokey-cornell-box", 1.0, 24, 24, 3, 50),  # media: the stream word keys the free path; Isotropic
    ("earth", 16 / 9, 32, 18, 2, 50),  # sphere uv into an image
    ("two-perlin-spheres", 16 / 9, 32, 18, 2, 50),
    ("textured-monument", 16 / 9, 32, 18, 2, 50),  # triangle uv
    ("book2-final-scene", 1.0, 24, 24, 2, 50),
])
def test_own_integrator_equals_the_oracle_render(gpu, orc, name, aspect, w, h, spp, max_depth):
    s = gpu.Scene()
    cam, bg = s.preset(name, aspect, seed=3)
    text, imgs = s.dump(), s.images()
    s.commit(device=0)
    ref, ref_rays = orc.OracleScene(text, imgs).render(orc.camera_from_fields(cam.as_dict()), bg, w, h, spp, seed=11,
                                                       max_depth=max_depth)
    img, nrays = _integrate(gpu, s, cam, bg, w, h, spp, 11, max_depth)
    assert nrays == ref_rays, f"ray count {nrays} vs oracle {ref_rays}"
    bad = np.argwhere(_bits(img) != _bits(ref))
    assert bad.size == 0, f"{len(bad)} mismatching components, first {bad[:4].tolist()}: " \
                          f"integrator {img[tuple(bad[0][:2])]} oracle {ref[tuple(bad[0][:2])]}"


# ---------------------------------------------------------------- 5. device forms
def test_device_forms_on_a_torch_stream_in_place(gpu):
    import torch
    w, h, spp, seed = 48, 27, 2, 11
    s = gpu.Scene()
    cam, bg = s.preset("jumpy-balls", 16 / 9, seed=3)
    s.commit(device=0)
    n = w * h * spp
    # the host forms, two bounces without compaction (a ray that ended is traced again from where it ended)
    r0 = s.camera_rays(cam, w, h, spp, seed, device=0)
    h0 = s.hit_rays(r0["origin"], r0["direction"], r0["time"], r0["stream"], device=0)
    r1, s0 = s.scatter_rays(r0, h0, bg, device=0)
    h1 = s.hit_rays(r1["origin"], r1["direction"], r1["time"], r1["stream"], device=0)
    r2, s1 = s.scatter_rays(r1, h1, bg, device=0)
    assert ((s0["flags"] & gpu.SCATTER_SCATTERED) != 0).sum() > n // 4 and (s0["flags"] == gpu.SCATTER_MISS).any()
    dev = torch.device("cuda:0")
    d_rays = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
    d_hits = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
    d_sc = [torch.zeros(n * 32, dtype=torch.uint8, device=dev) for _ in range(2)]
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        assert s.camera_rays_device(cam, w, h, spp, seed, 0, n, d_rays.data_ptr(), 0, stream.cuda_stream) is None
        got_r0 = d_rays.clone()
        for b in range(2):
            s.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, 0, stream.cuda_stream)
            s.scatter_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), bg, d_rays.data_ptr(), d_sc[b].data_ptr(), n, 0,
                                  stream.cuda_stream)  # out_rays = rays: in place
    stream.synchronize()
    _same_records(np.frombuffer(got_r0.cpu().numpy().tobytes(), gpu.RAY_DTYPE), r0, "camera rays")
    _same_records(np.frombuffer(d_sc[0].cpu().numpy().tobytes(), gpu.SCATTER_DTYPE), s0, "bounce 1")
    _same_records(np.frombuffer(d_sc[1].cpu().numpy().tobytes(), gpu.SCATTER_DTYPE), s1, "bounce 2")
    _same_records(np.frombuffer(d_rays.cpu().numpy().tobytes(), gpu.RAY_DTYPE), r2, "rays after two bounces")
    st = s.scatter_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), bg, d_rays.data_ptr(), d_sc[0].data_ptr(), n, 0,
                               stream.cuda_stream, want_stats=True)
    assert st["kernel_ms"] > 0 and st["total_ms"] > 0 and st["rays"] == 0 and st["paths"] == 0
    st = s.camera_rays_device(cam, w, h, spp, seed, 0, n, d_rays.data_ptr(), 0, stream.cuda_stream, want_stats=True)
    assert st["kernel_ms"] > 0 and st["total_ms"] > 0 and st["rays"] == 0 and st["paths"] == 0


# ---------------------------------------------------------------- 6. launch sizes
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_launches(gpu, orc, mat_scene, n):
    s, ids = mat_scene
    rays, hits, want_r, want_s, slot, _used = _block(gpu, orc, tuple(ids))
    out, sc = s.scatter_rays(rays[:n], hits[:n], BG, device=0)
    _same_records(sc, want_s[:n], f"n = {n}")
    _same_records(out[slot[:n] != 4], want_r[:n][slot[:n] != 4], f"n = {n}: out rays")


def test_second_staging_chunk(gpu, orc, mat_scene):
    """2^20 + 65 records through the host form: the block tiled, every copy's results equal to the first's."""
    s, ids = mat_scene
    rays, hits, want_r, want_s, slot, _used = _block(gpu, orc, tuple(ids))
    total, nb = (1 << 20) + 65, len(rays)
    reps = total // nb + 1
    out, sc, st = s.scatter_rays(np.tile(rays, reps)[:total], np.tile(hits, reps)[:total], BG, device=0,
                                 want_stats=True)
    assert len(out) == len(sc) == total and st["kernel_ms"] > 0 and st["rays"] == 0
    for got, size in ((out, 10), (sc, 8)):
        a = np.frombuffer(got.tobytes(), np.uint32).reshape(total, size)
        full = a[:(reps - 1) * nb].reshape(reps - 1, nb * size)
        bad = np.flatnonzero((full != full[0]).any(axis=1))
        assert bad.size == 0, f"copies {bad[:8].tolist()} differ from the first"
        tail = a[(reps - 1) * nb:]
        assert len(tail) > 65 and (tail == a[:len(tail)]).all(), "the last, partial copy (across the chunk boundary)"
    _same_records(sc[:nb], want_s, "first copy")
    _same_records(out[:nb][slot != 4], want_r[slot != 4], "first copy: out rays")


def test_camera_rays_second_staging_chunk(gpu):
    """2^20 + 65 paths from path 7 through the host form (two staging chunks; the second starts at first + 2^20) equal
    one rtw_camera_rays_device call for the range: a single launch without staging, of the kernel that
    test_camera_rays_match_the_oracle pins."""
    import torch
    w, h, spp, seed, first, n = 640, 410, 4, 11, 7, (1 << 20) + 65
    assert w * h * spp >= first + n
    s = gpu.Scene()
    cam, _bg = s.preset("jumpy-balls", 16 / 9, seed=3)
    s.commit(device=0)
    got, st = s.camera_rays(cam, w, h, spp, seed, first=first, n=n, device=0, want_stats=True)
    assert len(got) == n and st["kernel_ms"] > 0 and st["rays"] == 0
    dev = torch.device("cuda:0")
    d_rays = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
    s.camera_rays_device(cam, w, h, spp, seed, first, n, d_rays.data_ptr(), 0, 0)
    torch.cuda.synchronize(dev)
    _same_records(got, np.frombuffer(d_rays.cpu().numpy().tobytes(), gpu.RAY_DTYPE), "paths [7, 7 + 2^20 + 65)")
