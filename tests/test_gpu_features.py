"""Feature buffers on the GPU (rtw_render_features*: first-hit albedo, normal and depth per pixel, summed over the
pixel's camera rays by one fused kernel per scene variant).

Every comparison is bit for bit, on uint32 views.  The expected buffers are made without the feature: the rays come from
rtw_camera_rays (tests/test_gpu_scatter_rays.py holds it to the oracle), the hit and scatter records from the ORACLE
(OracleScene.hit_rays / .scatter_rays on the scene's dump, as tests/test_gpu_ray_corpus.py calls them); a sample's
albedo is `emitted` for a miss or a light and `attenuation` for a scattered record, and for a Metal record the colour
on that material's `metal` line of the dump (the text the oracle builds its materials from), absorbed or not; its
normal and (t, 1) are the hit record's, +0 and (0, 0) for a miss.  numpy sums them per pixel in sample order in
float32.  Each frame's expectation is made once, shared and never written."""
import functools
import subprocess

import numpy as np
import pytest

from test_gpu_far import assert_far, far_world

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED = 11
NAN_BITS = 0x7FC12345  # a quiet NaN no kernel computes: the sentinel of what must stay untouched
# (preset, w, h, spp): ragged on both axes, so edge tiles have off-image lanes
FRAMES = [
    ("jumpy-balls", 50, 27, 3),
    ("cornell-box", 26, 22, 4),
    ("smokey-cornell-box", 26, 22, 3),  # media: the stream word matters
    ("earth", 34, 18, 2),  # sphere uv into an image
    ("two-perlin-spheres", 34, 18, 2),
    ("textured-monument", 34, 18, 2),  # interpolated, unnormalised normals; triangle uv
    ("book2-final-scene", 26, 22, 2),
    ("wavefront-cow-obj", 34, 18, 2),
]
NAMES = ("albedo", "normal", "depth")
CH = {"albedo": 3, "normal": 3, "depth": 2}


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same(got, want, what):
    for n in want:
        if n not in got:
            continue
        g, w = _bits(got[n]), _bits(want[n])
        assert g.shape == w.shape, (what, n)
        bad = np.argwhere((g != w).reshape(g.shape[0], g.shape[1], -1).any(axis=2))
        assert bad.size == 0, f"{what}: {n} differs in {len(bad)} pixels, first {bad[0].tolist()}: " \
                              f"{got[n][tuple(bad[0])]} vs {want[n][tuple(bad[0])]}"


def _metal_colours(text):
    """material id -> float32 colour, from the dump's `mat K metal r g b fuzz` lines (C hex floats)"""
    out = {}
    for ln in text.splitlines():
        t = ln.split()
        if len(t) >= 6 and t[0] == "mat" and t[2] == "metal":
            out[int(t[1])] = np.array([float.fromhex(x) for x in t[3:6]], f32)
    return out


def expected(rtw, orc, s, text, imgs, cam, bg, w, h, spp, seed=SEED):
    """-> ({albedo, normal, depth} sums of samples [0, n) for every n <= spp as a list indexed by n, per-sample hit
    mask[h, w, spp]): the definition of include/rtw.h restated over the oracle's records."""
    rays = s.camera_rays(cam, w, h, spp, seed, device=0)  # path p = (row * w + i) * spp + s
    o = orc.OracleScene(text, imgs)
    hits = o.hit_rays(rays)
    sc = o.scatter_rays(rays, hits, bg)
    hit = (hits["flags"] & rtw.HIT_HIT) != 0
    scattered = (sc["flags"] & rtw.SCATTER_SCATTERED) != 0
    alb = np.where(scattered[:, None], sc["attenuation"], sc["emitted"]).astype(f32)
    assert (alb[~hit] == np.asarray(bg, f32)).all(), "a miss: the background"
    for m, colour in _metal_colours(text).items():
        alb[hit & (hits["material"] == m)] = colour
    nrm = np.where(hit[:, None], hits["normal"], f32(0)).astype(f32)
    dep = np.stack([np.where(hit, hits["t"], f32(0)), hit.astype(f32)], axis=1).astype(f32)
    per = {"albedo": alb.reshape(h, w, spp, 3), "normal": nrm.reshape(h, w, spp, 3), "depth": dep.reshape(h, w, spp, 2)}
    sums = [{n: np.zeros((h, w, CH[n]), f32) for n in NAMES}]
    with np.errstate(all="ignore"):
        for k in range(spp):
            nxt = {n: sums[-1][n] + per[n][:, :, k] for n in NAMES}
            assert all(v.dtype == f32 for v in nxt.values())
            sums.append(nxt)
    for d in sums:
        for v in d.values():
            v.setflags(write=False)
    return sums, hit.reshape(h, w, spp)


@functools.lru_cache(maxsize=None)
def _world(rtw, name, aspect):
    s = rtw.Scene()
    cam, bg = s.preset(name, aspect, seed=3)
    text, imgs = s.dump(), s.images()
    s.commit(device=0)
    return s, cam, bg, text, imgs


@functools.lru_cache(maxsize=None)
def _frame(rtw, orc, frame):
    name, w, h, spp = frame
    s, cam, bg, text, imgs = _world(rtw, name, w / h)
    sums, hit = expected(rtw, orc, s, text, imgs, cam, bg, w, h, spp)
    return s, cam, bg, sums, hit


# ---------------------------------------------------------------- 1. frames against the oracle
@pytest.mark.parametrize("frame", FRAMES, ids=[f[0] for f in FRAMES])
def test_frames_equal_the_oracle(gpu, orc, frame):
    name, w, h, spp = frame
    s, cam, bg, sums, hit = _frame(gpu, orc, frame)
    got, st = gpu.Raytracer(s, cam, bg, w, h, spp, seed=SEED).render_features()
    assert sorted(got) == sorted(NAMES) and got["depth"].shape == (h, w, 2)
    _same(got, sums[spp], name)
    assert st["rays"] == st["paths"] == w * h * spp and st["kernel_ms"] > 0 and st["total_ms"] > 0
    assert 0 < hit.sum(), "the frame hits something"
    assert (got["depth"][..., 1] == hit.sum(axis=2)).all(), "the second depth channel is the hit count"
    s.render_status(device=0)  # no guard trip


def _every_kind_world(rtw):
    """Every material kind on spheres, rects and triangles, a checker, and coincident duplicate spheres with another
    material, so that the tie rule (the later object) decides the albedo."""
    s = rtw.Scene()
    chk = s.lambertian(s.checker(s.solid_rgb(0.2, 0.3, 0.1), s.solid_rgb(0.9, 0.9, 0.9), 3.0))
    lam = s.lambertian_solid((0.7, 0.2, 0.1))
    met = s.metal((0.8, 0.6, 0.2), 0.9)  # a fuzzy Metal: many of its rays are absorbed
    met2 = s.metal((0.3, 0.9, 0.7), 0.0)
    die = s.dielectric(1.5)
    lit = s.diffuse_light(s.checker(s.solid_rgb(4.0, 1.0, 0.5), s.solid_rgb(0.5, 1.0, 4.0), 2.0))
    iso = s.isotropic(s.solid_rgb(0.4, 0.5, 0.6))
    mats = [chk, lam, met, met2, die, lit, iso]
    s.xz_rect(-6.0, 6.0, -6.0, 6.0, -1.0, chk)
    with s.bvh():
        for k, m in enumerate(mats):  # spheres of every kind ...
            s.sphere((-3.0 + k, 0.0, 0.0), 0.45, m)
        for k, (a, b) in enumerate(((lam, met), (met, lit), (die, iso))):  # ... and coincident pairs: the later wins
            s.sphere((-1.0 + k, 1.2, 0.3), 0.4, a)
            s.sphere((-1.0 + k, 1.2, 0.3), 0.4, b)
        for k, m in enumerate(mats):  # rects of every kind, standing behind
            s.xy_rect(-3.5 + k, -2.6 + k, 1.8, 2.6, -1.5, m)
        for k, m in enumerate(mats):  # triangles of every kind, in front
            x = -3.2 + 0.9 * k
            s.triangles([x, -0.9, 1.2, x + 0.7, -0.9, 1.2, x + 0.35, -0.3, 1.0], m)
    with s.constant_medium(1.5, s.solid_rgb(0.9, 0.9, 0.9)):
        s.sphere((2.5, 1.3, 0.5), 0.6, lam)
    text, imgs = s.dump(), s.images()
    s.commit(device=0)
    cam = rtw.Camera.new((0.3, 1.0, 7.0), (0.0, 0.6, 0.0), (0, 1, 0), 40.0, 29 / 19, 0.05, 7.0)
    return s, cam, text, imgs


def test_every_material_on_every_primitive_and_ties(gpu, orc):
    s, cam, text, imgs = _every_kind_world(gpu)
    bg, w, h, spp = (0.1, 0.2, 0.4), 29, 19, 3
    sums, hit = expected(gpu, orc, s, text, imgs, cam, bg, w, h, spp)
    got, st = gpu.Raytracer(s, cam, bg, w, h, spp, seed=SEED).render_features()
    _same(got, sums[spp], "every kind")
    assert st["rays"] == st["paths"] == w * h * spp
    # the world shows what it is for: every Metal colour, the white of glass and a light's colours are in the albedo
    one = expected(gpu, orc, s, text, imgs, cam, bg, w, h, 1)[0][1]["albedo"].reshape(-1, 3)
    seen = {tuple(v) for v in one.tolist()}
    key = lambda colour: tuple(np.asarray(colour, f32).tolist())
    for colour in ((0.8, 0.6, 0.2), (0.3, 0.9, 0.7), (1.0, 1.0, 1.0), (0.4, 0.5, 0.6)):
        assert key(colour) in seen, colour
    assert key((4.0, 1.0, 0.5)) in seen or key((0.5, 1.0, 4.0)) in seen, "a light's texture value"


# ---------------------------------------------------------------- the device form
def _device(gpu, s, cam, bg, w, h, first, n, bufs, ids=None, flags=0, stream=None, want_stats=False):
    """rtw_render_features_device onto the torch tensors in bufs (name -> tensor, missing = NULL)"""
    import torch
    rt = gpu.Raytracer(s, cam, bg, w, h, 1, seed=SEED)
    ptr = {k: (bufs[k].data_ptr() if k in bufs else 0) for k in NAMES}
    st = rt.render_features_device(ptr["albedo"], ptr["normal"], ptr["depth"], sample_first=first, n_samples=n,
                                   device=0, d_tiles_ptr=ids.data_ptr() if ids is not None else 0,
                                   n_tiles=len(ids) if ids is not None else 0,
                                   stream_ptr=stream.cuda_stream if stream is not None else 0, flags=flags,
                                   want_stats=want_stats)
    if stream is None:
        torch.cuda.synchronize()
    return st


def _zeros(w, h, names=NAMES):
    import torch
    return {k: torch.zeros((h, w, CH[k]), dtype=torch.float32, device="cuda:0") for k in names}


def _host(bufs):
    return {k: v.cpu().numpy() for k, v in bufs.items()}


# ---------------------------------------------------------------- 2. cuts
@pytest.mark.parametrize("name", ["jumpy-balls", "cornell-box"])
def test_cuts_subsets_and_no_samples(gpu, orc, name):
    import itertools
    import torch
    w, h, spp = (50, 27, 5) if name == "jumpy-balls" else (26, 22, 5)
    s, cam, bg, sums, _hit = _frame(gpu, orc, (name, w, h, spp))
    one = _zeros(w, h)
    st = _device(gpu, s, cam, bg, w, h, 0, 5, one, want_stats=True)
    assert st["rays"] == st["paths"] == w * h * 5
    _same(_host(one), sums[5], "[0, 5) in one call")
    cut = _zeros(w, h)
    for a, b in ((0, 1), (1, 3), (3, 5)):
        assert _device(gpu, s, cam, bg, w, h, a, b - a, cut) is None
        _same(_host(cut), sums[b], f"cut at {b}")
    host, _st = gpu.Raytracer(s, cam, bg, w, h, 5, seed=SEED).render_features()
    _same(host, _host(one), "the host form")
    # each non-empty subset of the three buffers gives the same bits for the buffers it names
    for r in (1, 2, 3):
        for names in itertools.combinations(NAMES, r):
            part = _zeros(w, h, names)
            _device(gpu, s, cam, bg, w, h, 0, 5, part)
            _same(_host(part), {k: sums[5][k] for k in names}, f"subset {names}")
            got, _st = gpu.Raytracer(s, cam, bg, w, h, 5, seed=SEED).render_features(want=names)
            assert sorted(got) == sorted(names)
            _same(got, {k: sums[5][k] for k in names}, f"host subset {names}")
    # n_samples = 0 touches nothing
    nan = {k: torch.full((h, w, CH[k]), 0, dtype=torch.int32, device="cuda:0").fill_(NAN_BITS).view(torch.float32)
           for k in NAMES}
    st = _device(gpu, s, cam, bg, w, h, 3, 0, nan, want_stats=True)
    assert st["rays"] == 0 and st["paths"] == 0
    for k in NAMES:
        assert (_bits(nan[k].cpu().numpy()) == NAN_BITS).all(), k


# ---------------------------------------------------------------- 3. tile sets
def test_tile_sets_packed_and_full_layout(gpu, orc):
    import torch
    name, w, h, spp = FRAMES[0]
    s, cam, bg, sums, _hit = _frame(gpu, orc, FRAMES[0])
    tx, nt = (w + 7) // 8, gpu.n_tiles(w, h)
    assert (tx, nt) == (7, 28) and w % 8 and h % 8
    # an interior tile, an ascending repeat-free subset, the ragged corner tile, one id equal to the tile count and one
    # far beyond it
    ids = [8, 1, 3, 9, 13, 20, nt - 1, nt, 0xFFFFFF00]
    assert len(set(ids)) == len(ids) and ids[1:6] == sorted(ids[1:6])
    d_ids = torch.from_numpy(np.asarray(ids, np.uint32).view(np.int32)).to("cuda:0")  # (uint32 bit patterns)
    want = sums[spp]

    def sentinel(shape):
        return torch.zeros(shape, dtype=torch.int32, device="cuda:0").fill_(NAN_BITS).view(torch.float32)

    # packed: [n_tiles][64][c].  The call adds: the named tiles' in-image slots start at +0, all else at the sentinel
    packed = {k: sentinel((len(ids), 64, CH[k])) for k in NAMES}
    for slot, t in enumerate(ids):
        if t < nt:
            ph, pw = min(8, h - (t // tx) * 8), min(8, w - (t % tx) * 8)
            for k in NAMES:
                packed[k][slot].view(8, 8, CH[k])[:ph, :pw] = 0.0
    st = _device(gpu, s, cam, bg, w, h, 0, spp, packed, ids=d_ids, want_stats=True)
    named_px = 0
    for slot, t in enumerate(ids):
        for k in NAMES:
            got = _bits(packed[k][slot].cpu().numpy()).reshape(8, 8, CH[k])
            if t >= nt:
                assert (got == NAN_BITS).all(), f"slot {slot} (id {t}) is skipped"
                continue
            r0, c0 = (t // tx) * 8, (t % tx) * 8
            ph, pw = min(8, h - r0), min(8, w - c0)
            assert (got[:ph, :pw] == _bits(want[k][r0:r0 + ph, c0:c0 + pw])).all(), (k, t)
            off = np.ones((8, 8), bool)
            off[:ph, :pw] = False
            assert (got[off] == NAN_BITS).all(), f"off-image slots of tile {t}"
        if t < nt:
            named_px += min(8, h - (t // tx) * 8) * min(8, w - (t % tx) * 8)
    assert st["rays"] == st["paths"] == named_px * spp
    # RTW_FLAG_FULL_IMAGE: the same ids, each tile at its place; samples [1, spp) onto the named tiles' sums of [0, 1)
    tile_of = (np.arange(h) // 8)[:, None] * tx + (np.arange(w) // 8)[None, :]
    named = np.isin(tile_of, [t for t in ids if t < nt])
    assert named.any() and not named.all() and named.sum() == named_px
    full = {k: sentinel((h, w, CH[k])) for k in NAMES}
    for k in NAMES:
        full[k][torch.from_numpy(named).to("cuda:0")] = torch.from_numpy(sums[1][k][named]).to("cuda:0")
    st = _device(gpu, s, cam, bg, w, h, 1, spp - 1, full, ids=d_ids, flags=gpu.FLAG_FULL_IMAGE, want_stats=True)
    assert st["rays"] == named_px * (spp - 1)
    for k in NAMES:
        got = _bits(full[k].cpu().numpy())
        assert (got[named] == _bits(want[k])[named]).all(), k
        assert (got[~named] == NAN_BITS).all(), f"{k}: tiles not named keep their sentinel"


# ---------------------------------------------------------------- 4. every walk
def _cfg(s):
    """rtw_scene_info 16-23: stack, spill, occ, feat, blk, ncap, half, s16 of the selected kernel"""
    return dict(zip(("stack", "spill", "occ", "feat", "blk", "ncap", "half", "s16"), (s.info(k) for k in range(16, 24))))


F_LIST = 1 << 16
F_ALL = ((1 << 16) - 1) | (1 << 17)
SPHERES, TRIANGLES, RECTS = FRAMES[0], FRAMES[7], FRAMES[1]
# tests/test_gpu_sample_rays.py's WALKS, restated
WALKS = [
    (SPHERES, None, dict(blk=1024, ncap=144, half=0, occ=8)),
    (SPHERES, "RTW_STACK_LDS=4", dict(stack=4, spill=1, feat=F_ALL)),
    (SPHERES, "RTW_LDS_NODES=0", dict(ncap=0, blk=256, occ=6)),
    (SPHERES, "RTW_HALF_NODES=1", dict(ncap=144, blk=512, half=1)),
    (SPHERES, "RTW_LDSN_BLK=512", dict(ncap=144, blk=512, half=0)),
    (SPHERES, "RTW_GENERIC=1,RTW_OCC=5", dict(feat=F_ALL, ncap=0, occ=5, blk=256)),
    (TRIANGLES, None, dict(s16=1, half=1, occ=7)),
    (TRIANGLES, "RTW_STACK_LDS=4", dict(stack=4, spill=1, feat=F_ALL)),
    (TRIANGLES, "RTW_MESH_S16=0", dict(s16=0, half=1, occ=5)),
    (TRIANGLES, "RTW_MESH_S16=6", dict(s16=1, half=1, occ=6)),
    (TRIANGLES, "RTW_GENERIC=1", dict(feat=F_ALL, s16=0, occ=5)),
    (RECTS, None, dict(feat=lambda f: f & F_LIST and f != (F_ALL | F_LIST), occ=8)),
    (RECTS, "RTW_LIST_ALL=1", dict(feat=F_ALL | F_LIST)),
    (RECTS, "RTW_GENERIC=1", dict(feat=F_ALL | F_LIST)),
]


@pytest.mark.parametrize("frame,knob,cfg", WALKS, ids=[f"{f[0]}-{k}" for f, k, _c in WALKS])
def test_every_walk_gives_the_expected_buffers(gpu, orc, knobs, frame, knob, cfg):
    name, w, h, spp = frame
    s, cam, bg, sums, _hit = _frame(gpu, orc, frame)  # (made once: the oracle knows no walk)
    for kv in (knob or "").split(","):
        if kv:
            knobs.setenv(*kv.split("="))
    have = _cfg(s)
    for k, v in cfg.items():
        assert v(have[k]) if callable(v) else have[k] == v, (knob, k, have)
    got, st = gpu.Raytracer(s, cam, bg, w, h, spp, seed=SEED).render_features()
    _same(got, sums[spp], f"{name} under {knob}")
    assert st["rays"] == st["paths"] == w * h * spp
    s.render_status(device=0)


# ---------------------------------------------------------------- 5. far origins
def test_far_origins_take_the_far_walk(gpu, orc):
    """tests/test_gpu_far.py's construction: the camera inside the r = 1000 ground sphere, 1,200 units under a field of
    small (some moving) balls, farther than D0 from them, so every camera ray reaches the BVH through trace_far."""
    s, text, imgs, cam = far_world(gpu, "moving")
    assert_far(s)
    assert s.info(14) == 1
    bg, w, h, spp = (0.7, 0.8, 1.0), 26, 21, 2
    sums, hit = expected(gpu, orc, s, text, imgs, cam, bg, w, h, spp)
    got, st = gpu.Raytracer(s, cam, bg, w, h, spp, seed=SEED).render_features()
    _same(got, sums[spp], "far camera")
    assert st["rays"] == w * h * spp and hit.all(), "inside the ground sphere every ray hits"
    s.render_status(device=0)


# ---------------------------------------------------------------- 6. between two renders on a torch stream
def test_device_form_between_two_renders_on_a_torch_stream(gpu, orc):
    import torch
    name, w, h, spp = SPHERES
    s, cam, bg, sums, _hit = _frame(gpu, orc, SPHERES)
    rt = gpu.Raytracer(s, cam, bg, w, h, spp, seed=SEED)
    alone, st_alone = rt.render()
    dev = torch.device("cuda:0")
    img = [torch.zeros((h, w, 3), dtype=torch.float32, device=dev) for _ in range(2)]
    bufs = _zeros(w, h)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        rt.render_device(img[0].data_ptr(), 0, stream_ptr=stream.cuda_stream)
        assert _device(gpu, s, cam, bg, w, h, 0, spp, bufs, stream=stream) is None
        rst = rt.render_device(img[1].data_ptr(), 0, stream_ptr=stream.cuda_stream, want_stats=True)
    stream.synchronize()
    for k in range(2):
        assert (_bits(img[k].cpu().numpy()) == _bits(alone)).all(), f"render {k + 1}"
    assert rst["rays"] == st_alone["rays"]
    _same(_host(bufs), sums[spp], "features between two renders")
    more = _zeros(w, h)
    st = _device(gpu, s, cam, bg, w, h, 0, spp, more, stream=stream, want_stats=True)
    _same(_host(more), sums[spp], "with stats")
    assert st["rays"] == st["paths"] == w * h * spp and st["kernel_ms"] > 0 and st["total_ms"] > 0


# ---------------------------------------------------------------- 7. the CLI
def test_console_writes_the_feature_images(gpu, tmp_path):
    from PIL import Image
    from test_integration_abi import ROOT
    exe = ROOT / "raytracer-weekend_amd" / "bin" / "rtw_console"
    w, spp = 32, 2
    h = gpu.image_height(w)
    subprocess.run([str(exe), "cornell-box", "-w", str(w), "-s", str(spp), "--features", "--models",
                    str(ROOT / "models")], check=True, cwd=tmp_path, capture_output=True, timeout=120)
    png = {k: np.asarray(Image.open(tmp_path / "render" / f"{k}_0000.png").convert("RGB"))
           for k in ("image", "albedo", "normal")}
    for k, v in png.items():
        assert v.shape == (h, w, 3) and v.dtype == np.uint8, k
    aspect = gpu.camera_aspect(w, h)
    s = gpu.Scene()
    _cam, bg = s.preset("cornell-box", aspect, seed=0)
    s.commit(device=0)
    cam = gpu.preset_cameras("cornell-box", aspect)[0]
    got, _st = gpu.Raytracer(s, cam, bg, w, h, spp, seed=0).render_features()
    assert np.array_equal(png["albedo"], gpu.tonemap(got["albedo"], spp))
    # the normal image, from its definition (rtw_console --help)
    n = got["normal"]
    with np.errstate(all="ignore"):
        ln = np.sqrt(n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1] + n[..., 2] * n[..., 2])[..., None]
        v = np.where(ln > 0, f32(0.5) + f32(0.5) * (n / ln), f32(0.5)).astype(f32)
    want = (f32(255.999) * np.clip(v, f32(0), f32(0.999))).astype(np.uint8)
    assert np.array_equal(png["normal"], want)
