"""The counting kernels (RTW_FLAG_COUNT_TRAVERSAL: pick_kernel<true>, a second instance of every path-kernel variant
with its own register allocation).  bench.py --full renders through them and reports their counters (phase_share,
simd_util, node_visits, the by-type primitive tests), so they must render what their plain twins render -- the
oracle's frame, bit for bit, with its ray count -- and count what the code says they count.  One world per kernel
family, and the global-node and spill kernels by knob."""
import numpy as np
import pytest

from test_gpu_far import BG as FAR_BG, F_ALL, F_BOXES, F_MEDIUM, F_MESHES, F_SMOKE, F_SPHERES, H as FAR_H, \
    SEED as FAR_SEED, SPP as FAR_SPP, W as FAR_W, far_reference, far_world, selected_kernel

pytestmark = pytest.mark.gpu

PRESETS = {
    # name: aspect, w, h, spp, list mode (no BVH: Scene.info(3) == 0)
    "jumpy-balls": (16 / 9, 64, 36, 4, False),          # the 1024-lane LDS-node kernel, sharded dispenser
    "cornell-box": (1.0, 40, 40, 8, True),              # the rect list kernel (start ring)
    "wavefront-cow-obj": (16 / 9, 48, 27, 3, False),    # the S16 mesh walk (rtw_kernel_mesh.hip)
    "smokey-cornell-box": (1.0, 32, 32, 6, True),       # 8 prims: the all-features list kernel, with media
    "two-perlin-spheres": (16 / 9, 48, 27, 3, True),    # 2 spheres: the all-features list kernel, noise textures
}
F_LIST = 1 << 16
LDSN_1024 = (16, 0, 8, F_SPHERES, 1024, 144, 0, 0)
MESH_S16 = (30, 0, 7, F_MESHES, 256, 0, 1, 1)
SPILL_TEST = (4, 1, 4, F_ALL, 256, 0, 0, 0)
LIST_ALL = (1, 0, 5, F_ALL | F_LIST, 256, 0, 0, 0)
# (world, knob): the kernel it selects (rtw_scene_info 16-23, see test_gpu_far.py SPHERE_KERNELS)
KERNELS = {
    ("jumpy-balls", ""): LDSN_1024,
    ("jumpy-balls", "RTW_LDS_NODES=0"): (24, 0, 6, F_SPHERES, 256, 0, 0, 0),
    ("jumpy-balls", "RTW_STACK_LDS=4"): SPILL_TEST,
    ("cornell-box", ""): (1, 0, 8, F_BOXES | F_LIST, 256, 0, 0, 0),
    ("cornell-box", "RTW_LIST_ALL=1"): LIST_ALL,
    ("wavefront-cow-obj", ""): MESH_S16,
    ("wavefront-cow-obj", "RTW_LDS_NODES=0"): MESH_S16,  # (the knob is the sphere kernels': the cow's kernel stays)
    ("wavefront-cow-obj", "RTW_STACK_LDS=4"): SPILL_TEST,
    ("smokey-cornell-box", ""): LIST_ALL,
    ("two-perlin-spheres", ""): LIST_ALL,
    ("far:static", ""): LDSN_1024,  # the far-camera ball field of test_gpu_far.py (trace_far's node visits counted)
    # that file's rect-and-media BVH: the F_SMOKE kernel (smokey-cornell-box is a list world)
    ("far:smoke", ""): (24, 0, 5, F_SMOKE, 256, 0, 0, 0),
}
CASES = list(KERNELS)
SEED = 11
_REF = {}  # preset name -> (oracle image, oracle rays): rendered once, shared, never written


def _world(rtw, orc, name):
    """-> (committed Scene, Raytracer, oracle image, oracle rays, list mode expected)."""
    if name.startswith("far:"):
        s, text, imgs, cam = far_world(rtw, name[4:])
        ref, rays = far_reference(orc, name[4:], text, imgs, cam)
        return s, rtw.Raytracer(s, cam, FAR_BG, FAR_W, FAR_H, FAR_SPP, seed=FAR_SEED), ref, rays, False
    aspect, w, h, spp, is_list = PRESETS[name]
    s = rtw.Scene()
    cam, bg = s.preset(name, aspect, seed=3)
    text, imgs = s.dump(), s.images()
    s.commit(device=0)
    if name not in _REF:
        ref, rays = orc.OracleScene(text, imgs).render(orc.camera_from_fields(cam.as_dict()), bg, w, h, spp, seed=SEED)
        ref.setflags(write=False)
        _REF[name] = (ref, rays)
    return (s, rtw.Raytracer(s, cam, bg, w, h, spp, seed=SEED)) + _REF[name] + (is_list,)


@pytest.mark.parametrize("world,knob", CASES)
def test_count_kernel_renders_and_counts(gpu, orc, knobs, world, knob):
    """The same frame through the plain kernel and through its COUNT twin: equal images (every bit), equal ray
    counts, both equal to the oracle's.  Then the counters, as far as the code fixes them:
      * prim_tests >= the sum of its by-type slots, equal without media (test_prim counts a ConstantMedium in the
        total only); a list world visits no node and tests no box; a BVH world does both, at most 4 boxes per node4
        visit (trace_far's visits count no boxes);
      * the wave cycles split into regeneration, traversal, shading and its sampling, one after the other, so each
        share is within [0, 1] and the four sum to at most 1; the sub-phases are timed inside them (start_path within
        regeneration, the node loop and the leaf tests within traversal) and cannot exceed them;
      * simd_util = active lanes / (64 x wave executions), within (0, 1] wherever anything was counted;
      * a plain render reports none of these;
      * RTW_LIST_ALL=1 (the all-features list kernel): trace_begin calls test_prim once per always-list primitive
        for every segment, and test_prim counts before any accept or early-out, so prim_tests = rays x n_always."""
    torch = pytest.importorskip("torch")
    rtw = gpu
    if knob:
        knobs.setenv(*knob.split("="))
    s, rt, ref, rays, is_list = _world(rtw, orc, world)
    assert (s.info(3) == 0) == is_list
    assert selected_kernel(s) == KERNELS[(world, knob)]
    if world == "far:smoke":
        assert s.info(9) & ~F_SMOKE == 0 and s.info(14) == 1
    stream = torch.cuda.current_stream().cuda_stream
    frames, stats = [], []
    for flags in (0, rtw.FLAG_COUNT_TRAVERSAL):
        out = torch.zeros((rt.h, rt.w, 3), dtype=torch.float32, device="cuda:0")
        stats.append(rt.render_device(out.data_ptr(), 0, 0, 0, stream, flags=flags, want_stats=True))
        frames.append(out.cpu().numpy())
    (plain, counted), (sp, sc) = frames, stats
    # C1: the same image and rays, and the oracle's
    assert sp["rays"] == sc["rays"] == rays, (sp["rays"], sc["rays"], rays)
    bad = np.argwhere((plain.view(np.uint32) != counted.view(np.uint32)).any(axis=2))
    assert bad.size == 0, f"COUNT differs from plain at {len(bad)} pixels, first {bad[:4].tolist()}"
    bad = np.argwhere((counted.view(np.uint32) != ref.view(np.uint32)).any(axis=2))
    assert bad.size == 0, f"{len(bad)} pixels differ from the oracle, first {bad[:4].tolist()}"
    # C2: the plain kernel counts nothing
    assert sp["node_visits"] == sp["prim_tests"] == sp["boxes_tested"] == 0 and not any(sp["prim_tests_by_type"])
    assert all(v is None for v in sp["simd_util"].values()) and all(v is None for v in sp["phase_share"].values())
    # ... and the COUNT kernel what the code says
    print(f"{world} {knob}: {sc}")
    by_type = sum(sc["prim_tests_by_type"])
    if s.info(9) & F_MEDIUM:
        assert sc["prim_tests"] > by_type > 0
    else:
        assert sc["prim_tests"] == by_type > 0
    if is_list:
        assert sc["node_visits"] == 0 and sc["boxes_tested"] == 0
        assert sc["simd_util"]["node_loop"] is None
    else:
        assert 0 < sc["boxes_tested"] <= 4 * sc["node_visits"]
    ph = sc["phase_share"]
    assert all(v is not None and 0.0 <= v <= 1.0 for v in ph.values()), ph
    assert ph["regen"] + ph["trace"] + ph["shade"] + ph["sample"] <= 1.0 + 1e-9, ph
    assert ph["regen"] > 0 and ph["trace"] > 0 and ph["shade"] > 0
    # the sub-phases are timed inside their phase, wave by wave: start_path within regeneration (rounds that start
    # no path included), the node loop and the leaf tests within traversal
    assert ph["path_start"] <= ph["regen"] + 1e-12, ph
    assert ph["node_loop"] + ph["leaf_tests"] <= ph["trace"] + 1e-12, ph
    for k, v in sc["simd_util"].items():
        assert v is None or 0.0 < v <= 1.0, (k, v)
    assert sc["simd_util"]["prim_tests"] is not None and sc["simd_util"]["segments"] is not None
    if knob == "RTW_LIST_ALL=1":
        assert s.info(5) == 18  # cornell-box: 6 rects and two Cuboids, all in the always list
        assert sc["prim_tests"] == sc["rays"] * s.info(5)
