"""The ray-query kernels (rtw_hit_rays, rtw_scatter_rays, rtw_sample_rays and their _device forms: hit_kernel,
scatter_kernel, sample_kernel) against the CPU oracle on rays no camera made, bit for bit.

tests/test_ray_corpus.py makes, per random world, 2,048 rays of fourteen classes (origins inside media, glass and
hollow spheres, on surfaces, in rect planes and on triangle edges; silhouette, axis-parallel, unnormalised and far
rays; the shutter's end times; stream words with a zero half) and the oracle's answers for them through
oracle_hit_rays / oracle_scatter_rays / oracle_sample_rays, which wrap the functions oracle_render is made of and share
no code with the kernels.  Here every ray of every world goes through the three host queries and is compared on uint32
views, NaN patterns and the sign of zero included; no ray is excluded at run time.  A ray that the oracle finds tied
(two objects at the winner's t exactly; at most TIE_CAP = 128 per world, asserted there on the CPU) is compared by hit
flag, t and material only in the hit records; its scatter and sample records are compared in full like any other.

The worlds: tests/test_gpu_fuzz.py's mixed worlds 0-5 and 329 (the NaN-throughput world) and two of its mesh worlds at
2,000 triangles, four of tests/test_sphere_fuzz_worlds.py's sphere worlds (cluster, bare, dome, offset).  RTW_RAY_SEEDS
raises the count (default 12 -> 13 worlds).

Measured on an MI355X: the module's 26 tests take 4.0 s in all (the oracle's answers included); the slowest world is
mesh-0 at 0.8 s (the oracle walks 2,000 triangles per segment), every other test is under 0.3 s.
One long run, RTW_RAY_SEEDS=120: 121 worlds, 247,808 rays, 218 tests in 23 s, no difference in any record.  The runs
before it found the two faults that the regression tests at the end of this module hold: unit() lost the sign of a zero
component (2 rays of the default worlds), and the first mend of it lost the sign of +0 / r for a hollow sphere's
negative r (1 ray of the long run)."""
import numpy as np
import pytest

from test_ray_corpus import CASES, DEPTH_SUBSET, N_RAYS, TIE_CAP, answers, build_world, case_id, corpus, same

pytestmark = pytest.mark.gpu

F_LIST = 1 << 16
F_ALL = ((1 << 16) - 1) | (1 << 17)
HIT_FIELDS = ("flags", "t", "p", "normal", "u", "v", "material")
SCATTER_FIELDS = ("flags", "attenuation", "emitted", "reserved")
RAY_FIELDS = ("origin", "direction", "time", "stream", "reserved")
SAMPLE_FIELDS = ("color", "segments", "stream", "flags", "reserved")
# the walks a world can take -> what rtw_scene_info 16-23 must then show (tests/test_gpu_sample_rays.py's WALKS)
WALKS = {
    "mixed": [("RTW_STACK_LDS=4", dict(stack=4, spill=1, feat=F_ALL))],
    "list": [("RTW_LIST_ALL=1", dict(feat=F_ALL | F_LIST))],
    "mesh": [("RTW_MESH_S16=0", dict(s16=0, half=1, occ=5)), ("RTW_STACK_LDS=4", dict(stack=4, spill=1, feat=F_ALL)),
             ("RTW_GENERIC=1", dict(feat=F_ALL, s16=0, occ=5))],
    "spheres": [("RTW_STACK_LDS=4", dict(stack=4, spill=1, feat=F_ALL)),
                ("RTW_GENERIC=1,RTW_OCC=5", dict(feat=F_ALL, ncap=0, occ=5, blk=256)),
                ("RTW_LDS_NODES=0", dict(ncap=0, blk=256, occ=6)), ("RTW_HALF_NODES=1", dict(ncap=144, blk=512, half=1))],
}
LIST_WORLD = ("mixed", 2)  # the default range's list-mode world (asserted below)
WALK_CASES = CASES[1::3] + [LIST_WORLD]  # a third of the worlds: a mixed, a mesh and a sphere world among them
DEVICE_CASE = ("mixed", 0)  # a medium, wrappers, every material


def _scene(gpu, case, knobs):
    """the world, committed under the environment of the moment (kernel variants are chosen per call)"""
    s, bg, _frame = build_world(gpu, case, knobs)
    s.commit(device=0)
    return s, bg


def _hits(s, rays):
    return s.hit_rays(rays["origin"], rays["direction"], rays["time"], rays["stream"], device=0)


def _check_hits(gpu, got, a, what):
    want, tie = a["hits"], a["tie"]
    assert got.dtype == gpu.HIT_DTYPE and tie.sum() <= TIE_CAP
    same(got[~tie], want[~tie], HIT_FIELDS, f"{what}: hit records")
    same(got[tie], want[tie], ("t", "material"), f"{what}: tied hit records")
    assert ((got["flags"][tie] & gpu.HIT_HIT) != 0).all()
    miss = (want["flags"] & gpu.HIT_HIT) == 0  # rtw.h: flags = 0, t = +inf and zeros elsewhere
    m = got[miss]
    assert (m["flags"] == 0).all() and np.isposinf(m["t"]).all() and (m["key"] == 0).all()


def _check_samples(got, st, want, what):
    same(got, want, SAMPLE_FIELDS, f"{what}: sample records")
    assert st["rays"] == int(want["segments"].astype(np.uint64).sum()) and st["paths"] == len(want), what


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_hit_scatter_and_sample_records_equal_the_oracle(gpu, orc, knobs, case):
    a = answers(gpu, orc, case, knobs)
    rays, _label = corpus(gpu, orc, case, knobs)
    s, bg = _scene(gpu, case, knobs)
    what = case_id(case)
    # 1. hits
    hits = _hits(s, rays)
    _check_hits(gpu, hits, a, what)
    # 2. scatter, on the GPU's own hit records
    out, sc = s.scatter_rays(rays, hits, bg, device=0)
    want = a["scene"].scatter_rays(rays, hits, bg)
    assert not (sc["flags"] & gpu.SCATTER_BAD).any()
    same(sc, want, SCATTER_FIELDS[:3], f"{what}: scatter records")
    assert (sc["reserved"] == 0).all() and (out["reserved"] == 0).all()
    same(out, want, RAY_FIELDS[:4], f"{what}: out rays")
    # 3. samples
    got, st = s.sample_rays(rays, bg, 50, device=0, want_stats=True)
    _check_samples(got, st, a["samples"][50], f"{what} at depth 50")
    for depth in (1, 2, 3):
        got, st = s.sample_rays(rays[:DEPTH_SUBSET], bg, depth, device=0, want_stats=True)
        _check_samples(got, st, a["samples"][depth], f"{what} at depth {depth}")
    s.render_status(device=0)  # no guard trip


def _cfg(s):
    """rtw_scene_info 16-23: stack, spill, occ, feat, blk, ncap, half, s16 of the selected kernel"""
    return dict(zip(("stack", "spill", "occ", "feat", "blk", "ncap", "half", "s16"), (s.info(k) for k in range(16, 24))))


def _walks():
    for case in WALK_CASES:
        for knob, cfg in WALKS["list" if case == LIST_WORLD else case[0]]:
            yield case, knob, cfg


@pytest.mark.parametrize("case,knob,cfg", list(_walks()), ids=[f"{case_id(c)}-{k}" for c, k, _ in _walks()])
def test_every_walk_equals_the_oracle(gpu, orc, knobs, case, knob, cfg):
    a = answers(gpu, orc, case, knobs)
    rays, _label = corpus(gpu, orc, case, knobs)
    s, bg = _scene(gpu, case, knobs)  # (committed under the default knobs, as the worlds above)
    base = _cfg(s)
    if case == LIST_WORLD:
        assert s.info(3) == 0 and base["feat"] & F_LIST, "list mode"
    for kv in knob.split(","):
        knobs.setenv(*kv.split("="))
    have = _cfg(s)
    for k, v in cfg.items():
        assert have[k] == v, (knob, k, have)
    assert have != base or case == LIST_WORLD, "the knob selects another kernel"
    what = f"{case_id(case)} under {knob}"
    _check_hits(gpu, _hits(s, rays), a, what)
    got, st = s.sample_rays(rays, bg, 50, device=0, want_stats=True)
    _check_samples(got, st, a["samples"][50], what)
    s.render_status(device=0)


def test_device_forms_on_a_torch_stream(gpu, orc, knobs):
    """The _device forms on a torch stream, the scattered rays written in place; and a launch of 65 rays cut from the
    middle of the corpus (a full wave and one lane), through both forms."""
    import torch
    case = DEVICE_CASE
    a = answers(gpu, orc, case, knobs)
    rays, _label = corpus(gpu, orc, case, knobs)
    s, bg = _scene(gpu, case, knobs)
    dev = torch.device("cuda:0")
    up = lambda rec: torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1).copy()).to(dev)
    down = lambda t, dtype: np.frombuffer(t.cpu().numpy().tobytes(), dtype)

    def run(r):
        n = len(r)
        d_rays, d_hits = up(r), torch.full((n * 48,), 0xAB, dtype=torch.uint8, device=dev)
        d_sc, d_smp = torch.full((n * 32,), 0xAB, dtype=torch.uint8, device=dev), torch.full((n * 32,), 0xAB, dtype=torch.uint8, device=dev)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            s.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, 0, stream.cuda_stream)
            s.sample_rays_device(d_rays.data_ptr(), bg, 50, d_smp.data_ptr(), n, 0, stream.cuda_stream)
            s.scatter_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), bg, d_rays.data_ptr(), d_sc.data_ptr(), n, 0,
                                  stream.cuda_stream)  # in place: the rays become the scattered rays
        stream.synchronize()
        return (down(d_hits, gpu.HIT_DTYPE), down(d_rays, gpu.RAY_DTYPE), down(d_sc, gpu.SCATTER_DTYPE),
                down(d_smp, gpu.SAMPLE_DTYPE))

    def check(r, sl, what):
        hits, out, sc, smp = run(r)
        want, tie = a["hits"][sl], a["tie"][sl]
        same(hits[~tie], want[~tie], HIT_FIELDS, f"{what}: hit records")
        same(hits[tie], want[tie], ("t", "material"), f"{what}: tied hit records")
        ws = a["scene"].scatter_rays(r, hits, bg)
        same(sc, ws, SCATTER_FIELDS[:3], f"{what}: scatter records")
        same(out, ws, RAY_FIELDS[:4], f"{what}: out rays, in place")
        same(smp, a["samples"][50][sl], SAMPLE_FIELDS, f"{what}: sample records")

    check(rays, slice(None), "device forms")
    mid = slice(N_RAYS // 2 - 32, N_RAYS // 2 + 33)
    assert mid.stop - mid.start == 65
    check(rays[mid], mid, "65 rays from the middle, device forms")
    part = rays[mid]
    hits = _hits(s, part)
    same(hits[~a["tie"][mid]], a["hits"][mid][~a["tie"][mid]], HIT_FIELDS, "65 rays from the middle: hit records")
    got, st = s.sample_rays(part, bg, 50, device=0, want_stats=True)
    _check_samples(got, st, a["samples"][50][mid], "65 rays from the middle")
    s.render_status(device=0)


def test_unit_keeps_the_sign_of_a_zero_component(gpu, orc, knobs):
    """The bug this corpus found.  Rays 875 and 1900 of world mixed-3 (class `axis`: directions (-0, -0, 1) and
    (-1, -0, 0)) are reflected inside a Dielectric sphere whose normal has y = -0.  vec3.rs:85-87 divides every
    component by the length, and -0 / |d| is -0, so the reflected direction's y is -0 - (+0) = -0; the kernels' unit()
    divided by Markstein's correction with the residual r = fma(-q0, |d|, x), under which a dividend of -0 came out as
    +0, and the out ray's y was +0.  First the division alone (rtw_diag_libm 4 is the kernels' div_by_recip), then the
    two rays through the scatter query and, sampled, through the fused kernel."""
    q = gpu.diag_libm(4, np.array([-0.0, 0.0, -0.0, 0.0], np.float32), np.array([3.0, 3.0, 0.75, 1e-3], np.float32))
    assert (q.view(np.uint32) == np.array([0x80000000, 0, 0x80000000, 0], np.uint32)).all(), q
    case = ("mixed", 3)
    a = answers(gpu, orc, case, knobs)
    rays, label = corpus(gpu, orc, case, knobs)
    s, bg = _scene(gpu, case, knobs)
    pick = np.array([875, 1900])
    r = rays[pick]
    assert (r["direction"][:, 1] == 0).all() and np.signbit(r["direction"][:, 1]).all()
    hits = _hits(s, r)
    same(hits, a["hits"][pick], HIT_FIELDS, "the two rays: hit records")
    assert (a["hits"]["normal"][pick][:, 1] == 0).all() and np.signbit(a["hits"]["normal"][pick][:, 1]).all()
    out, sc = s.scatter_rays(r, hits, bg, device=0)
    want = a["scatter"][pick]
    assert (want["direction"][:, 1] == 0).all() and np.signbit(want["direction"][:, 1]).all(), "the oracle: -0"
    assert (want["stream"] == r["stream"]).all(), "reflected because it cannot refract: nothing drawn"
    same(out, want, RAY_FIELDS[:4], "the two rays: out rays")
    same(sc, want, SCATTER_FIELDS[:3], "the two rays: scatter records")
    same(s.sample_rays(r, bg, 50, device=0), a["samples"][50][pick], SAMPLE_FIELDS, "the two rays: sample records")


def test_sphere_normal_keeps_the_sign_of_a_zero_component(gpu, orc):
    """spherical.rs:49 divides p - c by the radius, which is negative for a hollow sphere, and the hit record's
    division must keep a zero component's sign for either sign of it.  A long run's world (sphere world 24, a hollow
    shell at x = -2048.8525, where the coordinates are 2^-12 apart) had p.x == c.x: +0 / -0.45 = -0, where the
    correction from RN(1 / r) gave +0 once it was made right for positive divisors.  Here a solid and a hollow unit
    sphere and rays that stay in the plane x = c.x, from outside the solid one, where (p - c).x is -0 (o.x = d.x = -0),
    and from inside the hollow one, where it is +0: all four normals must carry -0."""
    s = gpu.Scene()
    m = s.lambertian_solid((0.5, 0.5, 0.5))
    s.sphere((0.0, 0.0, 0.0), 1.0, m)
    s.sphere((10.0, 0.0, 0.0), -1.0, m)
    text = s.dump()
    s.commit(device=0)
    o = np.array([[-0.0, 0.25, 3.0], [10.0, 0.25, 0.0], [-0.0, -0.5, -4.0], [10.0, -0.5, 0.125]], np.float32)
    d = np.array([[-0.0, 0.0, -1.0], [0.0, 0.2, -0.98], [-0.0, 0.1, 1.0], [-0.0, 0.3, 0.7]], np.float32)
    rays = gpu.make_rays(o, d, np.full(4, 0.5, np.float32), np.arange(1, 5, dtype=np.uint64))
    want = orc.OracleScene(text).hit_rays(rays)
    assert ((want["flags"] & gpu.HIT_HIT) != 0).all() and (want["normal"][:, 0] == 0).all()
    assert np.signbit(want["normal"][:, 0]).all(), "the oracle: -0 / 1 and +0 / -1 are -0, and all four face front"
    same(_hits(s, rays), want, HIT_FIELDS, "normals in the plane x = c.x")
