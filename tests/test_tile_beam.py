"""The beam test behind the per-tile lists of camera rays (csrc/rtw_tile_beam.h), on the CPU.

rtw_diag_tile_beam answers, for one camera, one 8x8 tile of a frame and one box, whether any camera ray of the tile can
meet the box.  The render relies on one property only: it never says "no" for a box that a ray of the tile does meet.
Here that is checked against an exact slab test in double over rays drawn in double from the reference's own
construction (camera.rs:66-74, lib.rs:84-85): origin + lens offset, towards llc + u horizontal + v vertical.

Rays take the extremes the margins have to cover: lens samples on the disk's rim, at its centre and at the corners of
its bounding square, pixel jitters 0 and the largest value below 1, the four corner pixels of a tile (of its on-image
part for a partial tile).  Tiles are the frame's four corners, its edges and its middle, on frames with partial tiles
on both edges.  Cameras are in focus (no lens) and defocused (lens radius 0.05 and 0.5), looking level, straight down
and from inside the boxes' cloud; boxes lie in front of, beside and behind the lens, and half of them are placed on a
ray of the tile so that enough pairs truly intersect (asserted, with the share of boxes the test rejects, so that
neither side of the property passes vacuously)."""
import numpy as np

FRAMES = [(64, 36), (20, 20), (13, 9), (1920, 1080)]
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


def _cameras(rtw):
    cams = []
    for lens in (0.0, 0.1, 1.0):  # aperture = 2 x lens radius
        cams.append(rtw.Camera.new((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 16 / 9, lens, 10.0))     # the preset's view
        cams.append(rtw.Camera.new((0, 9, 0.5), (0, 0, 0.5), (0, 0, -1), 60.0, 1.0, lens, 4.0))     # straight down
        cams.append(rtw.Camera.new((0.3, 0.4, -0.2), (5, 1, 2), (0, 1, 0), 90.0, 13 / 9, lens, 2.5))  # inside
        cams.append(rtw.Camera.new((-6, 1, 7), (1, 0.5, -1), (0.2, 1, 0.1), 35.0, 16 / 9, lens, 30.0))  # far focus
    return cams


def _tiles(w, h):
    tx, ty = (w + 7) // 8, (h + 7) // 8
    xs = sorted({0, tx // 2, tx - 1})
    ys = sorted({0, ty // 2, ty - 1})
    return [y * tx + x for y in ys for x in xs]


def _tile_rays(cam, w, h, tile, rng, n_random):
    """(origins, directions) in double of the tile's extreme rays and n_random random ones."""
    c = cam.c
    o, llc, hor, ver, cu, cv = (np.array(list(getattr(c, k)), np.float64)
                                for k in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v"))
    R = float(c.lens_radius)
    tx = (w + 7) // 8
    i0, r0 = (tile % tx) * 8, (tile // tx) * 8
    i1, r1 = min(i0 + 7, w - 1), min(r0 + 7, h - 1)
    s = np.sqrt(0.5)
    lens = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (s, s), (-s, s), (s, -s), (-s, -s),
            (1, 1), (1, -1), (-1, 1), (-1, -1)]  # centre, rim, and the bounding square's corners
    combos = [(i, r, jx, jy, a, b) for i in (i0, i1) for r in (r0, r1) for jx in (0.0, BELOW_ONE)
              for jy in (0.0, BELOW_ONE) for a, b in lens]
    for _ in range(n_random):
        ang, rad = rng.uniform(0, 2 * np.pi), np.sqrt(rng.uniform())
        combos.append((rng.integers(i0, i1 + 1), rng.integers(r0, r1 + 1), rng.uniform(), rng.uniform(),
                       rad * np.cos(ang), rad * np.sin(ang)))
    q = np.array(combos, np.float64)
    su = (q[:, 0] + q[:, 2]) / (w - 1)
    sv = ((h - 1 - q[:, 1]) + q[:, 3]) / (h - 1)
    A = o + R * q[:, 4:5] * cu + R * q[:, 5:6] * cv
    F = llc + su[:, None] * hor + sv[:, None] * ver
    return A, F - A


def _slab_hits(A, D, lo, hi):
    """Exact slab test in double, t >= 0: rays [n, 3] against boxes [m, 3] -> bool [m, n]."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (lo[:, None, :] - A[None]) / D[None]
        t1 = (hi[:, None, :] - A[None]) / D[None]
    # a zero direction component: inside the slab -> unconstrained, outside -> miss
    zero = (D == 0)[None]
    inside = (A[None] >= lo[:, None, :]) & (A[None] <= hi[:, None, :])
    tn = np.where(zero, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1))
    tf = np.where(zero, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1))
    return np.maximum(tn.max(axis=2), 0.0) <= tf.min(axis=2)


def test_beam_never_rejects_a_box_that_a_ray_meets(rtw):
    rng = np.random.default_rng(11)
    pairs = meeting = boxes = rejected = 0
    for ci, cam in enumerate(_cameras(rtw)):
        w, h = FRAMES[ci % len(FRAMES)]
        for tile in _tiles(w, h):
            A, D = _tile_rays(cam, w, h, tile, rng, 12)
            n_box = 6
            # half the boxes on a ray of the tile (in front of, at and beyond the focus plane), the others anywhere
            # around the camera: beside and behind the lens too
            k = rng.integers(0, len(A), n_box)
            t = rng.choice([0.02, 0.3, 1.0, 2.5, 8.0], n_box) * rng.uniform(0.5, 1.5, n_box)
            on_ray = A[k] + t[:, None] * D[k] + rng.normal(0, 0.02, (n_box, 3)) * np.linalg.norm(D[k], axis=1)[:, None]
            around = np.array(list(cam.c.origin)) + rng.normal(0, 6.0, (n_box, 3))
            ctr = np.where((np.arange(n_box) % 2 == 0)[:, None], on_ray, around)
            half = rng.choice([0.01, 0.2, 1.5], n_box)[:, None] * rng.uniform(0.2, 1.0, (n_box, 3))
            lo, hi = (ctr - half).astype(np.float32), (ctr + half).astype(np.float32)
            hit = _slab_hits(A, D, lo.astype(np.float64), hi.astype(np.float64))
            for b in range(n_box):
                may = rtw.diag_tile_beam(cam, w, h, tile, lo[b], hi[b])
                boxes += 1
                rejected += not may
                pairs += hit.shape[1]
                meeting += int(hit[b].sum())
                assert may or not hit[b].any(), \
                    f"camera {ci} {w}x{h} tile {tile}: box {lo[b]}..{hi[b]} rejected, but ray " \
                    f"{A[hit[b]][0]} + t {D[hit[b]][0]} meets it"
    assert pairs >= 100_000, pairs
    assert meeting >= 10_000, f"only {meeting} of {pairs} (ray, box) pairs intersect: the property was barely tested"
    assert rejected >= boxes // 5, f"the beam test rejected {rejected} of {boxes} boxes: it culls nothing"


def test_beam_on_the_preset_view(rtw):
    """The shape of the estimate the lists rest on: under the jumpy-balls camera at 1080p a 0.2 ball's box is a
    candidate of the tile it projects to and of few others."""
    cam = rtw.Camera.new((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 16 / 9, 0.1, 10.0)
    w, h = 1920, 1080
    lo, hi = np.float32([3.8, 0.0, 0.8]), np.float32([4.2, 0.4, 1.2])
    n = sum(rtw.diag_tile_beam(cam, w, h, t, lo, hi) for t in range(rtw.n_tiles(w, h)))
    assert 1 <= n <= 0.02 * rtw.n_tiles(w, h), n
