"""Which path kernel a world and a knob set select (rtw_kernel.hip pick_kernel, rtw_variants.hpp pick5,
rtw_kernel_mesh.hip pick_mesh), asserted.

rtw_scene_info 16-23 report the KernelCfg that the current environment selects for a committed scene; no device is
needed.  The table below was recorded from the commit before the selection code was restructured (that commit plus
the introspection call alone, which read the template arguments out of the selected kernel's mangled name), so it pins
the selection as it was: a knob that quietly falls through to the default kernel, or a rule that moves, fails here.
tests/test_gpu_far.py and tests/test_gpu_count.py assert the same for the kernels they render with."""
import numpy as np
import pytest

from test_gpu_far import WORLDS as FAR_WORLDS, SPHERE_KNOBS, F_SPHERES, F_BOXES, F_SMOKE, F_MESHES, _ball_field

F_ALL = ((1 << 16) - 1) | (1 << 17)
F_LIST = 1 << 16

# (stack, spill, occ, feat, blk, ncap, half, s16): rtw_scene_info 16-23, KernelCfg's fields in order
CFG = {
    "boxes_24_occ5": (24, 0, 5, F_BOXES, 256, 0, 0, 0),
    "boxes_24_occ5_spill": (24, 1, 5, F_BOXES, 256, 0, 0, 0),
    "spheres_ldsn512x144": (16, 0, 8, F_SPHERES, 512, 144, 0, 0),
    "spheres_ldsn512x144_half": (16, 0, 8, F_SPHERES, 512, 144, 1, 0),
    "spheres_ldsn1024x144": (16, 0, 8, F_SPHERES, 1024, 144, 0, 0),
    "spheres_ldsn448x160": (18, 0, 7, F_SPHERES, 448, 160, 0, 0),
    "spheres_ldsn448x160_half": (18, 0, 7, F_SPHERES, 448, 160, 1, 0),
    "spheres_24_occ5": (24, 0, 5, F_SPHERES, 256, 0, 0, 0),
    "spheres_24_occ6": (24, 0, 6, F_SPHERES, 256, 0, 0, 0),
    "spheres_ldsn512x224": (24, 0, 6, F_SPHERES, 512, 224, 0, 0),
    "spheres_ldsn512x224_half": (24, 0, 6, F_SPHERES, 512, 224, 1, 0),
    "spheres_24_occ5_spill": (24, 1, 5, F_SPHERES, 256, 0, 0, 0),
    "spheres_32_occ4": (32, 0, 4, F_SPHERES, 256, 0, 0, 0),
    "spheres_32_occ4_spill": (32, 1, 4, F_SPHERES, 256, 0, 0, 0),
    "smoke_24_occ5": (24, 0, 5, F_SMOKE, 256, 0, 0, 0),
    "list_boxes_occ6": (1, 0, 6, F_BOXES | F_LIST, 256, 0, 0, 0),
    "list_boxes_occ8": (1, 0, 8, F_BOXES | F_LIST, 256, 0, 0, 0),
    "mesh_24_occ5": (24, 0, 5, F_MESHES, 256, 0, 0, 0),
    "mesh_24_occ5_half": (24, 0, 5, F_MESHES, 256, 0, 1, 0),
    "mesh_30_occ5": (30, 0, 5, F_MESHES, 256, 0, 0, 0),
    "mesh_30_occ5_half": (30, 0, 5, F_MESHES, 256, 0, 1, 0),
    "mesh_s16_occ6": (30, 0, 6, F_MESHES, 256, 0, 0, 1),
    "mesh_s16_occ6_half": (30, 0, 6, F_MESHES, 256, 0, 1, 1),
    "mesh_s16_occ7": (30, 0, 7, F_MESHES, 256, 0, 0, 1),
    "mesh_s16_occ7_half": (30, 0, 7, F_MESHES, 256, 0, 1, 1),
    "mesh_30_occ5_spill": (30, 1, 5, F_MESHES, 256, 0, 0, 0),
    "spill_test": (4, 1, 4, F_ALL, 256, 0, 0, 0),
    "all_24_occ5": (24, 0, 5, F_ALL, 256, 0, 0, 0),
    "all_30_occ5": (30, 0, 5, F_ALL, 256, 0, 0, 0),
    "all_30_occ5_spill": (30, 1, 5, F_ALL, 256, 0, 0, 0),
    "all_32_occ4": (32, 0, 4, F_ALL, 256, 0, 0, 0),
    "all_32_occ4_spill": (32, 1, 4, F_ALL, 256, 0, 0, 0),
    "list_all_occ5": (1, 0, 5, F_ALL | F_LIST, 256, 0, 0, 0),
}

PARITY_KNOBS = ["RTW_REGEN_MIN=1", "RTW_REGEN_MIN=64", "RTW_QUOTA16=1", "RTW_QUOTA16=16", "RTW_LIST_MAX=0",
                "RTW_LIST_MAX=64", "RTW_LIST_OCC=6", "RTW_LEAF16=1", "RTW_LEAF16=16", "RTW_LDS_NODES=0", "RTW_OCC=5",
                "RTW_HALF_NODES=1", "RTW_HALF_NODES=0", "RTW_TRI_LEAF=0", "RTW_LDSN_WAVES=6", "RTW_LDSN_WAVES=7",
                "RTW_LDSN_BLK=512", "RTW_MESH_S16=0", "RTW_MESH_S16=6", "RTW_MESH_S16=7", "RTW_BVH_PAIR=1",
                "RTW_BVH_BINS=64", "RTW_BATCH=64", "RTW_BATCH=65536", "RTW_BATCH=100", "RTW_BATCH=1000"]
COUNT_KNOBS = ["RTW_LDS_NODES=0", "RTW_STACK_LDS=4", "RTW_LIST_ALL=1"]
# tests/test_gpu_parity.py test_scheduling_knobs_bit_exact, tests/test_gpu_far.py SPHERE_KNOBS, tests/test_gpu_count.py
# and pairs of them for the returns no single knob reaches
PAIR_KNOBS = ["RTW_HALF_NODES=0,RTW_MESH_S16=7", "RTW_HALF_NODES=0,RTW_MESH_S16=6", "RTW_LIST_MAX=0,RTW_MESH_S16=0",
              "RTW_HALF_NODES=1,RTW_LDSN_WAVES=7", "RTW_HALF_NODES=1,RTW_LDSN_WAVES=6", "RTW_LIST_MAX=0,RTW_OCC=4"]
KNOBS = list(dict.fromkeys(SPHERE_KNOBS + PARITY_KNOBS + COUNT_KNOBS + PAIR_KNOBS))
# the knobs the flattener reads (rtw_flatten.cpp): a scene is committed once per setting of these
FLATTEN_KNOBS = ("RTW_LIST_MAX", "RTW_TRI_LEAF", "RTW_BVH_PAIR", "RTW_BVH_BINS")


def _preset(name, aspect):
    return lambda rtw, s: s.preset(name, aspect, seed=3)


def _far(name):
    seed, make = FAR_WORLDS[name]
    return lambda rtw, s: make(rtw, s, np.random.default_rng(seed))


def _balls(n, seed):
    """test_gpu_far's static ball field with n x n balls: sphere worlds past each LDS node table's capacity."""
    return lambda rtw, s: _ball_field(rtw, s, np.random.default_rng(seed), n=n, moving=False)


def _chain(n, g, rotated=False):
    """n spheres on a line, centre and radius growing by the factor g: the SAH tree splits one off at a time, so
    the traversal-stack bound passes the LDS stacks' 24 / 30 / 32 rows with few nodes (the SPILL kernels)."""
    def make(rtw, s):
        m = s.lambertian_solid((0.5, 0.5, 0.5))
        c = np.array([(g ** k, 0.0, 0.0) for k in range(n)], np.float32)
        r = np.array([0.1 * g ** k for k in range(n)], np.float32)
        if rotated:
            with s.rotate_y(10.0):
                s.spheres(c, r, [m] * n)
        else:
            s.spheres(c, r, [m] * n)
    return make


def _rect_chain(n, g, fog=False):
    """The same chain of n rects (a deep rect BVH: the F_BOXES SPILL kernel), with one sphere-bounded medium the
    F_SMOKE one."""
    def make(rtw, s):
        m = s.lambertian_solid((0.5, 0.5, 0.5))
        for k in range(n):
            s.xy_rect(0.0, 0.1 * g ** k, 0.0, 0.1 * g ** k, g ** k, m)
        if fog:
            with s.constant_medium(1.0, s.solid_rgb(0.5, 0.5, 0.5)):
                s.sphere((0.0, 0.0, -2.0), 0.5, m)
    return make


def _quad_mesh(rtw, s):
    """test_gpu_far's mesh world without its balls: 72 triangles in the BVH and none of the sphere tests that would
    send it to the generic kernel (a small mesh tree: the 24-row mesh kernels)."""
    ground = s.lambertian(s.checker(s.solid_rgb(0.2, 0.3, 0.1), s.solid_rgb(0.9, 0.9, 0.9), 10.0))
    s.sphere((0, -1000, 0), 1000, ground)
    p = np.linspace(-2.0, 2.0, 7, dtype=np.float32)
    v = lambda i, j: (p[i], 0.05 + 0.1 * (p[i] + 2.0), p[j])
    tris = []
    for i in range(6):
        for j in range(6):
            tris += [v(i, j), v(i + 1, j), v(i + 1, j + 1), v(i, j), v(i + 1, j + 1), v(i, j + 1)]
    s.triangles(np.array(tris, np.float32).ravel(), s.lambertian_solid((0.6, 0.4, 0.3)))


WORLDS = {
    "jumpy-balls": _preset("jumpy-balls", 16 / 9),
    "cornell-box": _preset("cornell-box", 1.0),
    "smokey-cornell-box": _preset("smokey-cornell-box", 1.0),
    "wavefront-cow-obj": _preset("wavefront-cow-obj", 16 / 9),
    "textured-monument": _preset("textured-monument", 16 / 9),
    "book2-final-scene": _preset("book2-final-scene", 1.0),
    "two-perlin-spheres": _preset("two-perlin-spheres", 16 / 9),
    "far:static": _far("static"),
    "far:moving": _far("moving"),
    "far:rotated": _far("rotated"),
    "far:mesh": _far("mesh"),
    "far:smoke": _far("smoke"),
    "far:tall": _far("tall"),
    "balls:147": _balls(23, 2),   # node4s: past the 1024 / 512-lane table (144)
    "balls:170": _balls(24, 24),  # past the 448-lane table (160)
    # (far:tall, 254 node4s: past the 224 of the 6-wave table)
    "chain:80": _chain(80, 1.2),
    "chain:80:rotated": _chain(80, 1.2, rotated=True),
    "chain:300": _chain(300, 1.06),
    "chain:300:rotated": _chain(300, 1.06, rotated=True),
    "rect-chain:80": _rect_chain(80, 1.2),
    "quad-mesh": _quad_mesh,
}
# world -> (the configuration selected without knobs and by every knob set of KNOBS not named here, {knob set: the
# configuration it selects instead})
TABLE = {
    "jumpy-balls": ("spheres_ldsn1024x144", {
        "RTW_LDS_NODES=0": "spheres_24_occ6", "RTW_HALF_NODES=1": "spheres_ldsn512x144_half",
        "RTW_LDSN_WAVES=6": "spheres_ldsn512x224", "RTW_LDSN_WAVES=7": "spheres_ldsn448x160",
        "RTW_LDSN_BLK=512": "spheres_ldsn512x144", "RTW_OCC=5": "spheres_24_occ5", "RTW_OCC=4": "spheres_32_occ4",
        "RTW_GENERIC=1,RTW_OCC=5": "all_24_occ5", "RTW_STACK_LDS=4": "spill_test",
        "RTW_BVH_PAIR=1": "spheres_24_occ6", "RTW_HALF_NODES=1,RTW_LDSN_WAVES=7": "spheres_ldsn448x160_half",
        "RTW_HALF_NODES=1,RTW_LDSN_WAVES=6": "spheres_ldsn512x224_half",
        "RTW_LIST_MAX=0,RTW_OCC=4": "spheres_32_occ4",
    }),
    "cornell-box": ("list_boxes_occ8", {
        "RTW_GENERIC=1": "list_all_occ5", "RTW_GENERIC=1,RTW_OCC=5": "list_all_occ5",
        "RTW_STACK_LDS=4": "spill_test", "RTW_LIST_MAX=0": "boxes_24_occ5", "RTW_LIST_OCC=6": "list_boxes_occ6",
        "RTW_LIST_ALL=1": "list_all_occ5", "RTW_LIST_MAX=0,RTW_MESH_S16=0": "boxes_24_occ5",
        "RTW_LIST_MAX=0,RTW_OCC=4": "all_32_occ4",
    }),
    "smokey-cornell-box": ("list_all_occ5", {
        "RTW_STACK_LDS=4": "spill_test", "RTW_LIST_MAX=0": "smoke_24_occ5",
        "RTW_LIST_MAX=0,RTW_MESH_S16=0": "smoke_24_occ5", "RTW_LIST_MAX=0,RTW_OCC=4": "all_32_occ4",
    }),
    "wavefront-cow-obj": ("mesh_s16_occ7_half", {
        "RTW_OCC=4": "all_32_occ4", "RTW_GENERIC=1": "all_30_occ5", "RTW_GENERIC=1,RTW_OCC=5": "all_30_occ5",
        "RTW_STACK_LDS=4": "spill_test", "RTW_HALF_NODES=0": "mesh_30_occ5",
        "RTW_MESH_S16=0": "mesh_30_occ5_half", "RTW_MESH_S16=6": "mesh_s16_occ6_half",
        "RTW_HALF_NODES=0,RTW_MESH_S16=7": "mesh_s16_occ7", "RTW_HALF_NODES=0,RTW_MESH_S16=6": "mesh_s16_occ6",
        "RTW_LIST_MAX=0,RTW_MESH_S16=0": "mesh_30_occ5_half", "RTW_LIST_MAX=0,RTW_OCC=4": "all_32_occ4",
    }),
    "textured-monument": ("mesh_s16_occ7_half", {
        "RTW_OCC=4": "all_32_occ4", "RTW_GENERIC=1": "all_30_occ5", "RTW_GENERIC=1,RTW_OCC=5": "all_30_occ5",
        "RTW_STACK_LDS=4": "spill_test", "RTW_HALF_NODES=0": "mesh_30_occ5",
        "RTW_MESH_S16=0": "mesh_30_occ5_half", "RTW_MESH_S16=6": "mesh_s16_occ6_half",
        "RTW_BVH_PAIR=1": "mesh_30_occ5_spill", "RTW_HALF_NODES=0,RTW_MESH_S16=7": "mesh_s16_occ7",
        "RTW_HALF_NODES=0,RTW_MESH_S16=6": "mesh_s16_occ6", "RTW_LIST_MAX=0,RTW_MESH_S16=0": "mesh_30_occ5_half",
        "RTW_LIST_MAX=0,RTW_OCC=4": "all_32_occ4",
    }),
    "book2-final-scene": ("all_24_occ5", {
        "RTW_OCC=4": "all_32_occ4", "RTW_STACK_LDS=4": "spill_test", "RTW_LIST_MAX=0,RTW_OCC=4": "all_32_occ4",
    }),
    "two-perlin-spheres": ("list_all_occ5", {
        "RTW_STACK_LDS=4": "spill_test", "RTW_LIST_MAX=0": "all_24_occ5",
        "RTW_LIST_MAX=0,RTW_MESH_S16=0": "all_24_occ5", "RTW_LIST_MAX=0,RTW_OCC=4": "all_32_occ4",
    }),
    "far:static": ("spheres_ldsn1024x144", {
        "RTW_LDS_NODES=0": "spheres_24_occ6", "RTW_HALF_NODES=1": "spheres_ldsn512x144_half",
        "RTW_LDSN_WAVES=6": "spheres_ldsn512x224", "RTW_LDSN_WAVES=7": "spheres_ldsn448x160",
        "RTW_LDSN_BLK=512": "spheres_ldsn512x144", "RTW_OCC=5": "spheres_24_occ5", "RTW_OCC=4": "spheres_32_occ4",
        "RTW_GENERIC=1,RTW_OCC=5": "all_24_occ5", "RTW_STACK_LDS=4": "spill_test",
        "RTW_HALF_NODES=1,RTW_LDSN_WAVES=7": "spheres_ldsn448x160_half",
        "RTW_HALF_NODES=1,RTW_LDSN_WAVES=6": "spheres_ldsn512x224_half",
        "RTW_LIST_MAX=0,RTW_OCC=4": "spheres_32_occ4",
    }),
    "far:moving": ("spheres_ldsn1024x144", {
        "RTW_LDS_NODES=0": "spheres_24_occ6", "RTW_HALF_NODES=1": "spheres_ldsn512x144_half",
        "RTW_LDSN_WAVES=6": "spheres_ldsn512x224", "RTW_LDSN_WAVES=7": "spheres_ldsn448x160",
        "RTW_LDSN_BLK=512": "spheres_ldsn512x144", "RTW_OCC=5": "spheres_24_occ5", "RTW_OCC=4": "spheres_32_occ4",
        "RTW_GENERIC=1,RTW_OCC=5": "all_24_occ5", "RTW_STACK_LDS=4": "spill_test",
        "RTW_HALF_NODES=1,RTW_LDSN_WAVES=7": "spheres_ldsn448x160_half",
        "RTW_HALF_NODES=1,RTW_LDSN_WAVES=6": "spheres_ldsn512x224_half",
        "RTW_LIST_MAX=0,RTW_OCC=4": "spheres_32_occ4",
    }),
    "far:rotated": ("all_24_occ5", {
        "RTW_OCC=4": "all_32_occ4", "RTW_STACK_LDS=4": "spill_test", "RTW_LIST_MAX=0,RTW_OCC=4": "all_32_occ4",
    }),
    "far:mesh": ("all_24_occ5", {
        "RTW_OCC=4": "all_32_occ4", "RTW_STACK_LDS=4": "spill_test", "RTW_LIST_MAX=0,RTW_OCC=4": "all_32_occ4",
    }),
    "far:smoke": ("smoke_24_occ5", {
        "RTW_OCC=4": "all_32_occ4", "RTW_GENERIC=1": "all_24_occ5", "RTW_GENERIC=1,RTW_OCC=5": "all_24_occ5",
        "RTW_STACK_LDS=4": "spill_test", "RTW_LIST_MAX=64": "list_all_occ5",
        "RTW_LIST_MAX=0,RTW_OCC=4": "all_32_occ4",
    }),
    "far:tall": ("spheres_24_occ6", {
        "RTW_OCC=5": "spheres_24_occ5", "RTW_OCC=4": "spheres_32_occ4", "RTW_GENERIC=1,RTW_OCC=5": "all_24_occ5",
        "RTW_STACK_LDS=4": "spill_test", "RTW_LIST_MAX=0,RTW_OCC=4": "spheres_32_occ4",
    }),
    "balls:147": ("spheres_ldsn512x224", {
        "RTW_LDS_NODES=0": "spheres_24_occ6", "RTW_HALF_NODES=1": "spheres_ldsn512x224_half",
        "RTW_LDSN_WAVES=7": "spheres_ldsn448x160", "RTW_OCC=5": "spheres_24_occ5", "RTW_OCC=4": "spheres_32_occ4",
        "RTW_GENERIC=1,RTW_OCC=5": "all_24_occ5", "RTW_STACK_LDS=4": "spill_test",
        "RTW_BVH_PAIR=1": "spheres_24_occ6", "RTW_HALF_NODES=1,RTW_LDSN_WAVES=7": "spheres_ldsn448x160_half",
        "RTW_HALF_NODES=1,RTW_LDSN_WAVES=6": "spheres_ldsn512x224_half",
        "RTW_LIST_MAX=0,RTW_OCC=4": "spheres_32_occ4",
    }),
    "balls:170": ("spheres_ldsn512x224", {
        "RTW_LDS_NODES=0": "spheres_24_occ6", "RTW_HALF_NODES=1": "spheres_ldsn512x224_half",
        "RTW_OCC=5": "spheres_24_occ5", "RTW_OCC=4": "spheres_32_occ4", "RTW_GENERIC=1,RTW_OCC=5": "all_24_occ5",
        "RTW_STACK_LDS=4": "spill_test", "RTW_BVH_PAIR=1": "spheres_24_occ6",
        "RTW_HALF_NODES=1,RTW_LDSN_WAVES=7": "spheres_ldsn512x224_half",
        "RTW_HALF_NODES=1,RTW_LDSN_WAVES=6": "spheres_ldsn512x224_half",
        "RTW_LIST_MAX=0,RTW_OCC=4": "spheres_32_occ4",
    }),
    "chain:80": ("spheres_24_occ5_spill", {
        "RTW_OCC=4": "spheres_32_occ4", "RTW_GENERIC=1": "all_30_occ5", "RTW_GENERIC=1,RTW_OCC=5": "all_30_occ5",
        "RTW_STACK_LDS=4": "spill_test", "RTW_BVH_BINS=64": "spheres_24_occ6",
        "RTW_LIST_MAX=0,RTW_OCC=4": "spheres_32_occ4",
    }),
    "chain:80:rotated": ("all_30_occ5", {
        "RTW_OCC=4": "all_32_occ4", "RTW_STACK_LDS=4": "spill_test", "RTW_BVH_BINS=64": "all_24_occ5",
        "RTW_LIST_MAX=0,RTW_OCC=4": "all_32_occ4",
    }),
    "chain:300": ("spheres_24_occ5_spill", {
        "RTW_OCC=4": "spheres_32_occ4_spill", "RTW_GENERIC=1": "all_30_occ5_spill",
        "RTW_GENERIC=1,RTW_OCC=5": "all_30_occ5_spill", "RTW_STACK_LDS=4": "spill_test",
        "RTW_LIST_MAX=0,RTW_OCC=4": "spheres_32_occ4_spill",
    }),
    "chain:300:rotated": ("all_30_occ5_spill", {
        "RTW_OCC=4": "all_32_occ4_spill", "RTW_STACK_LDS=4": "spill_test",
        "RTW_LIST_MAX=0,RTW_OCC=4": "all_32_occ4_spill",
    }),
    "rect-chain:80": ("boxes_24_occ5_spill", {
        "RTW_OCC=4": "all_32_occ4_spill", "RTW_GENERIC=1": "all_30_occ5_spill",
        "RTW_GENERIC=1,RTW_OCC=5": "all_30_occ5_spill", "RTW_STACK_LDS=4": "spill_test",
        "RTW_LIST_MAX=0,RTW_OCC=4": "all_32_occ4_spill",
    }),
    "quad-mesh": ("mesh_s16_occ7_half", {
        "RTW_OCC=4": "all_32_occ4", "RTW_GENERIC=1": "all_24_occ5", "RTW_GENERIC=1,RTW_OCC=5": "all_24_occ5",
        "RTW_STACK_LDS=4": "spill_test", "RTW_HALF_NODES=0": "mesh_24_occ5",
        "RTW_MESH_S16=0": "mesh_24_occ5_half", "RTW_MESH_S16=6": "mesh_s16_occ6_half",
        "RTW_HALF_NODES=0,RTW_MESH_S16=7": "mesh_s16_occ7", "RTW_HALF_NODES=0,RTW_MESH_S16=6": "mesh_s16_occ6",
        "RTW_LIST_MAX=0,RTW_MESH_S16=0": "mesh_24_occ5_half", "RTW_LIST_MAX=0,RTW_OCC=4": "all_32_occ4",
    }),
}
_SCENES = {}  # (world, the flattener's knobs) -> committed Scene: built once, shared, only read


def _commit_anywhere(rtw, s):
    if rtw.device_count() > 0:
        s.commit()
    else:
        with pytest.raises(rtw.RtwError):
            s.commit()


def selected(rtw, world, knob, setenv, delenv):
    """The configuration `knob` (comma-separated NAME=VALUE, or "") selects for `world`."""
    kv = [k.split("=") for k in knob.split(",")] if knob else []
    for k, v in kv:
        setenv(k, v)
    key = (world,) + tuple((k, v) for k, v in kv if k in FLATTEN_KNOBS)
    if key not in _SCENES:
        s = rtw.Scene()
        WORLDS[world](rtw, s)
        _commit_anywhere(rtw, s)
        _SCENES[key] = s
    got = tuple(_SCENES[key].info(16 + f) for f in range(8))
    for k, _ in kv:
        delenv(k)
    return got


@pytest.mark.parametrize("world", list(WORLDS))
def test_selected_kernel(rtw, knobs, world):
    """Every (world, knob set) row selects the configuration the table names."""
    dflt, other = TABLE[world]
    assert set(other) <= set(KNOBS)
    bad = []
    for knob in KNOBS:
        want = other.get(knob, dflt)
        got = selected(rtw, world, knob, knobs.setenv, knobs.delenv)
        if got != CFG[want]:
            bad.append((knob, want, got))
    assert not bad, bad


def test_knobs_need_the_gate(rtw, monkeypatch):
    """Without RTW_TUNING=1 a knob selects nothing: the default kernel."""
    monkeypatch.delenv("RTW_TUNING", raising=False)
    for world in ("jumpy-balls", "wavefront-cow-obj"):
        for knob in ("RTW_OCC=4", "RTW_STACK_LDS=4", "RTW_GENERIC=1,RTW_OCC=5"):
            assert selected(rtw, world, knob, monkeypatch.setenv, monkeypatch.delenv) == CFG[TABLE[world][0]]


def test_every_reachable_return_is_hit():
    """pick_kernel, pick5 and pick_mesh return 34 configurations (two returns of pick_kernel's list branch name the
    same one); the table reaches all but the F_SMOKE kernel with the HBM stack spill, which needs a rect-and-media
    tree with a stack bound above 24 rows."""
    hit = {d for d, _ in TABLE.values()} | {c for _, o in TABLE.values() for c in o.values()}
    assert hit == set(CFG) and len(CFG) == 33
    assert len(set(CFG.values())) == 33


def test_mesh_s16_warning_only_where_consulted(rtw, knobs, capfd):
    """A value of RTW_MESH_S16 that no variant has is reported and replaced by the default, and only a mesh world
    consults the knob at all."""
    capfd.readouterr()
    assert selected(rtw, "jumpy-balls", "RTW_MESH_S16=5", knobs.setenv, knobs.delenv) == CFG[TABLE["jumpy-balls"][0]]
    assert "RTW_MESH_S16" not in capfd.readouterr().err
    assert selected(rtw, "quad-mesh", "RTW_MESH_S16=5", knobs.setenv, knobs.delenv) == CFG["mesh_s16_occ7_half"]
    assert "rtw: RTW_MESH_S16=5 ignored (0, 6 or 7)" in capfd.readouterr().err
