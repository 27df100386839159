"""Progressive renders on the GPU (rtw_render_samples_device, rtw_render_progressive, rtw_tonemap_device,
rtw_console --progressive): a frame's samples in chunks are the frame, bit for bit and ray for ray.

The path generator is keyed by (seed, j, i, sample) and a frame is the in-order f32 sum over its samples, so samples
[a, b) added onto the sums of [0, a) are rtw_render's frame of b samples however [0, b) is cut.  Every comparison is on
uint32 views.  References, each made once per frame and never changed: rtw_render's one-shot frame, the oracle's frame,
the sums and sums of squares after each of the chunks [0,1) [1,2) [2,4) [4,8) [8,13), and the per-sample records of
rtw_sample_rays over rtw_camera_rays.  The frames are tests/test_gpu_sample_rays.py's small ones, one per kernel family:
jumpy-balls 48x27 (the 1024-lane ring kernel with tile lists; 27 rows leave a partial tile row), cornell-box 24x24 at
depth 50 and 3 (the rect list kernel), smokey-cornell-box 24x24 (media sub-streams keyed by the path word) and
wavefront-cow-obj 32x18 (the S16 mesh walk)."""
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32
FRAMES = [
    ("jumpy-balls", 16 / 9, 48, 27, 50),
    ("cornell-box", 1.0, 24, 24, 50),
    ("cornell-box", 1.0, 24, 24, 3),  # depth exhaustion
    ("smokey-cornell-box", 1.0, 24, 24, 50),
    ("wavefront-cow-obj", 16 / 9, 32, 18, 50),
]
IDS = [f"{f[0]}-d{f[4]}" for f in FRAMES]
SEED, SPP = 11, 13
CHUNKS = [(0, 1), (1, 1), (2, 2), (4, 4), (8, 5)]  # (first, n): the prefixes 1, 2, 4, 8, 13
SENTINEL = np.array([0x7FC0BEEF], np.uint32).view(f32)[0]  # a NaN with a payload: any arithmetic on it shows


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same(got, want, what):
    a, b = _bits(got).reshape(-1), _bits(want).reshape(-1)
    assert a.shape == b.shape, what
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} components differ, first at {bad[0]}: " \
                          f"{np.ravel(got)[bad[0]]!r} vs {np.ravel(want)[bad[0]]!r}"


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _stream():
    return _torch().cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _world(rtw, name, aspect):
    s = rtw.Scene()
    cam, bg = s.preset(name, aspect, seed=3)
    text, imgs = s.dump(), s.images()
    s.commit(device=0)
    return s, cam, bg, text, imgs


def _tracer(rtw, frame, spp=SPP):
    name, aspect, w, h, depth = frame
    s, cam, bg, _t, _i = _world(rtw, name, aspect)
    return rtw.Raytracer(s, cam, bg, w, h, spp, seed=SEED, max_depth=depth)


def _render_ranges(rtw, frame, ranges, with_sq=True):
    """The ranges in order from zeroed device buffers -> [(sums, sums of squares or None, rays) after each]."""
    _n, _a, w, h, _d = frame
    rt = _tracer(rtw, frame)
    d_sum = _dev(np.zeros((h, w, 3), f32))
    d_sq = _dev(np.zeros((h, w, 3), f32)) if with_sq else None
    out = []
    for first, n in ranges:
        st = rt.render_samples_device(d_sum.data_ptr(), d_sq.data_ptr() if with_sq else 0, first, n, device=0,
                                      stream_ptr=_stream(), want_stats=True)
        assert st["paths"] == rtw.n_tiles(w, h) * 64 * n  # whole tiles, as rtw_render_device counts them
        out.append((d_sum.cpu().numpy(), d_sq.cpu().numpy() if with_sq else None, st["rays"]))
    return out


@functools.lru_cache(maxsize=None)
def _oneshot(rtw, frame):
    img, st = _tracer(rtw, frame).render()
    img.setflags(write=False)
    return img, st["rays"]


@functools.lru_cache(maxsize=None)
def _oracle(rtw, orc, frame, spp):
    name, aspect, w, h, depth = frame
    _s, cam, bg, text, imgs = _world(rtw, name, aspect)
    ref, rays = orc.OracleScene(text, imgs).render(orc.camera_from_fields(cam.as_dict()), bg, w, h, spp, seed=SEED,
                                                   max_depth=depth)
    ref.setflags(write=False)
    return ref, rays


@functools.lru_cache(maxsize=None)
def _prefixes(rtw, frame):
    """{samples done: (sums, sums of squares, rays of that chunk)} after each of CHUNKS"""
    snaps = _render_ranges(rtw, frame, CHUNKS)
    for a, b, _r in snaps:
        a.setflags(write=False)
        b.setflags(write=False)
    return {first + n: snap for (first, n), snap in zip(CHUNKS, snaps)}


@functools.lru_cache(maxsize=None)
def _prefix(rtw, frame, n):
    """(sums, sums of squares) of samples [0, n): CHUNKS' where it is one of their prefixes, else one call."""
    pre = _prefixes(rtw, frame)
    return pre[n][:2] if n in pre else _render_ranges(rtw, frame, [(0, n)])[0][:2]


# ---------------------------------------------------------------- 1, 2: chunks, prefixes
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_chunked_equals_one_shot_and_the_oracle(gpu, orc, frame):
    rtw = gpu
    pre = _prefixes(rtw, frame)
    img, rays = _oneshot(rtw, frame)
    ref, ref_rays = _oracle(rtw, orc, frame, SPP)
    _same(pre[SPP][0], img, "chunks 1+1+2+4+5 vs rtw_render")
    _same(pre[SPP][0], ref, "chunks 1+1+2+4+5 vs the oracle")
    assert sum(r for _a, _b, r in pre.values()) == rays == ref_rays
    for step in (3, 5):  # unaligned chunks: several blocks each
        ranges = [(a, min(step, SPP - a)) for a in range(0, SPP, step)]
        snaps = _render_ranges(rtw, frame, ranges)
        _same(snaps[-1][0], img, f"steps of {step} vs rtw_render")
        _same(snaps[-1][1], pre[SPP][1], f"steps of {step}: the sums of squares vs the chunks'")
        assert sum(r for _a, _b, r in snaps) == rays


@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_a_prefix_is_a_smaller_frame(gpu, orc, frame):
    rtw = gpu
    (got, _sq, rays), = _render_ranges(rtw, frame, [(0, 7)])
    ref, ref_rays = _oracle(rtw, orc, frame, 7)
    _same(got, ref, "[0, 7) vs the oracle at 7 spp")
    assert rays == ref_rays


# ---------------------------------------------------------------- 3: a range from the middle, the second moment
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_a_middle_range_and_its_second_moment(gpu, frame):
    """[5, 11) from zeroed buffers against the per-sample records: rtw_sample_rays over the camera rays of samples
    5..10 of a 16-spp frame (a path's key holds its sample index, not the frame's spp), summed in order in float32;
    the sums of squares likewise as m = m + x * x, two roundings."""
    rtw = gpu
    name, aspect, w, h, depth = frame
    s, cam, bg, _t, _i = _world(rtw, name, aspect)
    rays = s.camera_rays(cam, w, h, 16, SEED, device=0).reshape(h, w, 16)[:, :, 5:11]
    rec, st = s.sample_rays(rays.reshape(-1), bg, depth, device=0, want_stats=True)
    x = rec["color"].reshape(h, w, 6, 3)
    assert x.dtype == f32
    want, want_sq = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32)
    with np.errstate(all="ignore"):
        for k in range(6):
            want = want + x[:, :, k]
            want_sq = want_sq + x[:, :, k] * x[:, :, k]
    assert want.dtype == want_sq.dtype == f32
    (got, got_sq, n_rays), = _render_ranges(rtw, frame, [(5, 6)])
    _same(got, want, "[5, 11) vs the records' sums")
    _same(got_sq, want_sq, "[5, 11) vs the records' sums of squares")
    assert n_rays == st["rays"]
    (alone, none, n_alone), = _render_ranges(rtw, frame, [(5, 6)], with_sq=False)
    assert none is None and n_alone == n_rays
    _same(alone, want, "[5, 11) without d_sq")


# ---------------------------------------------------------------- 4, 5: what is left untouched
def test_tile_subsets_leave_the_rest_untouched(gpu):
    """jumpy-balls 48x27: 6 x 4 tiles, the last tile row with 3 of its 8 pixel rows in the image.  Packed layout: an id
    table with padding ids (= the tile count) between real ones; the buffers hold the sentinel but for the named
    tiles' pixels, which start at zero.  Full layout: the frame, with a sentinel tail behind it."""
    rtw = gpu
    frame = FRAMES[0]
    _n, _a, w, h, _d = frame
    rt = _tracer(rtw, frame)
    full, full_sq = _prefix(rtw, frame, SPP)
    nt, tiles_x = rtw.n_tiles(w, h), (w + 7) // 8
    assert (nt, tiles_x) == (24, 6)
    ids = np.array([3, 23, nt, 0, 20, nt, 11], np.uint32)
    lane = np.arange(64)
    start = np.full((len(ids), 64, 3), SENTINEL, f32)
    inside = np.zeros((len(ids), 64), bool)
    px = np.zeros((len(ids), 64, 2), np.int64)
    for k, t in enumerate(ids):
        if t < nt:
            row, col = (t // tiles_x) * 8 + lane // 8, (t % tiles_x) * 8 + lane % 8
            inside[k] = (row < h) & (col < w)
            px[k, :, 0], px[k, :, 1] = row, col
    assert inside[0].all() and inside[1].sum() == inside[4].sum() == 24 and not inside[2].any()
    start[inside] = 0.0
    d_ids, d_sum, d_sq = _dev(ids.view(np.int32)), _dev(start), _dev(start)
    for first, n in ((0, 4), (4, 9)):
        rt.render_samples_device(d_sum.data_ptr(), d_sq.data_ptr(), first, n, device=0, d_tiles_ptr=d_ids.data_ptr(),
                                 n_tiles=len(ids), stream_ptr=_stream())
    _torch().cuda.synchronize()
    for got, want, what in ((d_sum.cpu().numpy(), full, "sums"), (d_sq.cpu().numpy(), full_sq, "sums of squares")):
        _same(got[inside], want[px[inside][:, 0], px[inside][:, 1]], f"packed {what}: the named tiles")
        assert (_bits(got[~inside]) == _bits(SENTINEL)).all(), f"packed {what}: a pixel outside the named tiles changed"
    # the full layout: the whole frame, nothing behind it
    tail = 4096
    start = np.full(h * w * 3 + tail, SENTINEL, f32)
    start[:h * w * 3] = 0.0
    d_sum, d_sq = _dev(start), _dev(start)
    for first, n in ((0, 4), (4, 9)):
        rt.render_samples_device(d_sum.data_ptr(), d_sq.data_ptr(), first, n, device=0, stream_ptr=_stream())
    _torch().cuda.synchronize()
    for got, want, what in ((d_sum.cpu().numpy(), full, "sums"), (d_sq.cpu().numpy(), full_sq, "sums of squares")):
        _same(got[:h * w * 3], want, f"full layout {what}")
        assert (_bits(got[h * w * 3:]) == _bits(SENTINEL)).all(), f"full layout {what}: written behind the frame"


@pytest.mark.parametrize("nothing", ["max_depth", "n_samples"])
def test_nothing_to_do_leaves_the_buffers_untouched(gpu, nothing):
    rtw = gpu
    name, aspect, w, h, depth = FRAMES[0]
    s, cam, bg, _t, _i = _world(rtw, name, aspect)
    rt = rtw.Raytracer(s, cam, bg, w, h, SPP, seed=SEED, max_depth=0 if nothing == "max_depth" else depth)
    start = np.full((h, w, 3), SENTINEL, f32)
    start[::2] = -0.0  # x + 0 would turn these into +0
    d_sum, d_sq = _dev(start), _dev(start)
    st = rt.render_samples_device(d_sum.data_ptr(), d_sq.data_ptr(), 3, 0 if nothing == "n_samples" else 5, device=0,
                                  stream_ptr=_stream(), want_stats=True)
    assert st["rays"] == 0
    _same(d_sum.cpu().numpy(), start, "sums")
    _same(d_sq.cpu().numpy(), start, "sums of squares")


# ---------------------------------------------------------------- 6: rtw_render_progressive
@pytest.mark.parametrize("step,dones", [(0, [1, 2, 4, 8, 13]), (4, [1, 2, 4, 8, 12, 13])])
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_render_progressive_steps(gpu, frame, step, dones):
    rtw = gpu
    rt = _tracer(rtw, frame)
    seen = []
    rc, st = rt.render_progressive(lambda a, b, done: seen.append((done, a, b)), step)
    assert rc == 0 and [d for d, _a, _b in seen] == dones
    for done, a, b in seen:
        want, want_sq = _prefix(rtw, frame, done)
        _same(a, want, f"the sums after {done} samples")
        _same(b, want_sq, f"the sums of squares after {done} samples")
    img, rays = _oneshot(rtw, frame)
    _same(seen[-1][1], img, "the last frame vs rtw_render")
    assert st["rays"] == rays and st["paths"] == frame[2] * frame[3] * SPP


def test_render_progressive_sink_stops_the_render(gpu):
    rtw = gpu
    rt = _tracer(rtw, FRAMES[0])
    seen = []

    def on_frame(_a, _b, done):
        seen.append(done)
        return 7 if len(seen) == 3 else 0
    rc, st = rt.render_progressive(on_frame)
    assert rc == 7 and seen == [1, 2, 4]
    assert st["paths"] == FRAMES[0][2] * FRAMES[0][3] * 4
    assert st["rays"] == sum(_prefixes(rtw, FRAMES[0])[n][2] for n in (1, 2, 4))


# ---------------------------------------------------------------- 7: rtw_tonemap_device
@pytest.mark.parametrize("spp", [1, 13, 50])
def test_tonemap_device_equals_the_host_tonemap(gpu, spp):
    rtw = gpu
    rng = np.random.default_rng(spp)
    tiny = np.array([1, 2, 0x7FFFFF, 0x800000, 0x80000001, 0x807FFFFF], np.uint32).view(f32)  # denormals, the least normal
    crafted = np.concatenate([
        [0.0, -0.0, -1.0, -1e-30, -np.inf, np.inf, np.nan, -np.nan, spp, spp * 0.998, spp * 0.9981, spp * 1.5, 1e30],
        tiny, tiny * f32(spp), [spp * (k / 255.999) ** 2 for k in range(256)],
        rng.uniform(-1, 1.2 * spp, 3000), rng.uniform(0, 1e-3, 500)]).astype(f32)
    crafted = crafted[:(len(crafted) // 3) * 3].reshape(-1, 3)
    assert len(crafted) % 256 != 0 and len(crafted) > 1024  # several blocks, a partial last one
    want = rtw.tonemap(crafted, spp)
    d_sum = _dev(crafted)
    d_rgb = _torch().full((len(crafted) + 16, 3), 0xA5, dtype=_torch().uint8, device="cuda:0")
    rtw.tonemap_device(d_sum.data_ptr(), len(crafted), spp, d_rgb.data_ptr(), device=0, stream_ptr=_stream())
    _torch().cuda.synchronize()
    got = d_rgb.cpu().numpy()
    assert np.array_equal(got[:len(crafted)], want)
    assert (got[len(crafted):] == 0xA5).all(), "written behind the image"
    assert len(set(want.reshape(-1).tolist())) > 200  # the cases span the byte range


# ---------------------------------------------------------------- 8: the console front end
def test_console_progressive_png_is_the_one_shot_png(gpu, tmp_path):
    """`rtw_console jumpy-balls -w 48 -s 13 --progressive 4`: the steps 1, 2, 4, 8, 12, 13 on stdout, each with the
    frame's mean relative standard error, and a final PNG byte-identical to the run without the flag."""
    rtw = gpu
    exe = ROOT / "raytracer-weekend_amd" / "bin" / "rtw_console"
    assert exe.exists(), "rtw_console not built"
    base = [str(exe), "jumpy-balls", "-w", "48", "-s", "13", "--seed", "3", "--models", str(rtw.MODELS_DIR)]
    outs = {}
    for tag, extra in (("plain", []), ("progressive", ["--progressive", "4"])):
        d = tmp_path / tag
        r = subprocess.run(base + ["--out", str(d)] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert [p.name for p in sorted(d.glob("image_*.png"))] == ["image_0000.png"]
        outs[tag] = ((d / "image_0000.png").read_bytes(), r.stdout)
    assert outs["plain"][0] == outs["progressive"][0]
    lines = [ln.split() for ln in outs["progressive"][1].splitlines() if "standard error" in ln]
    assert [int(ln[0]) for ln in lines] == [1, 2, 4, 8, 12, 13]
    errs = [float(ln[-1]) for ln in lines[1:]]
    assert all(0.0 < e < 10.0 for e in errs) and errs[-1] < errs[0], errs  # the noise estimate falls with the samples
    assert "standard error" not in outs["plain"][1]
