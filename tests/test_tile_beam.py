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
neither side of the property passes vacuously).

A second test draws its rays in f32, by the oracle's own Camera::get_ray, from cameras shifted by 2^8, 2^11 and 2^14:
the rounding the margins exist for (32 u M (1 + t), M the largest magnitude).  Measured on scratch builds of the header:
it fails with BEAM_MARGIN at 3e-8 and below and passes from 1e-7 up (the f32 ray's two sums of M-sized terms stray
about 2 u M t, a sixteenth of the bound), so a margin cut by 1,000, to 2.5e-7, is still sound and no ray can show it;
with `z1 < -az` replaced by `z1 <= 0` it fails on the skewed-lens camera at 2^8."""
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


def _shifted_cameras(rtw):
    """Views whose eye and target are shifted by 2^8, 2^11 and 2^14 (M, the largest magnitude of the margin argument,
    is then the shift), with lens radius 0, 0.5 and 2: the preset's view, a view from inside the boxes' cloud, and one
    focused 2 units away at vfov 20, whose lens (radius 0.5 and 2) is wider than its focus cone
    (2 tan 10 deg = 0.35); and the preset's view with a skewed lens.  -> [(camera, focus distance)]"""
    cams = []
    for k, sign in ((8, (1, 1, -1)), (11, (-1, 1, 1)), (14, (1, -1, 1))):
        off = np.array(sign, np.float64) * np.array([2.0 ** k, 2.0 ** k / 4, 2.0 ** k])
        for lens in (0.0, 0.5, 2.0):
            for eye, at, vup, vfov, aspect, focus in (((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 16 / 9, 10.0),
                                                      ((0.3, 0.4, -0.2), (5, 1, 2), (0.2, 1, 0.1), 90.0, 13 / 9, 2.5),
                                                      ((-6, 1, 7), (1, 0.5, -1), (0, 1, 0), 20.0, 16 / 9, 2.0)):
                cams.append((rtw.Camera.new(tuple(np.array(eye) + off), tuple(np.array(at) + off), vup, vfov, aspect,
                                            2.0 * lens, focus), focus))
            if lens:
                # a skewed lens: u leans towards the view axis (rtw_camera is plain data, and the beam test assumes
                # no orthogonality), so part of the lens lies behind the plane through the origin: a box just
                # behind that plane is met by rays that start farther back (the `z1 < -az` rejection)
                cam = rtw.Camera.new(tuple(np.array((13, 2, 3)) + off), tuple(off), (0, 1, 0), 20.0, 16 / 9, 2.0 * lens, 10.0)
                u = np.array(list(cam.c.u), np.float64) + 0.5 * np.array(list(cam.c.w), np.float64)
                cam.c.u[:] = [float(x) for x in (u / np.linalg.norm(u)).astype(np.float32)]
                cams.append((cam, 10.0))
    return cams


def _f32_tile_rays(orc, cam, w, h, tile):
    """(origins, directions) as the oracle's own Camera::get_ray forms them in f32 (oracle_get_ray, camera.rs:66-74),
    with s, t formed in f32 as lib.rs:84-85 does: the tile's corner pixels, jitters 0 and the largest value below 1,
    lens draws at the centre, next to the rim on both axes and on the diagonals."""
    import ctypes as C
    f32 = np.float32
    L = orc.lib()
    ocam = orc.camera_from_fields(cam.as_dict())
    tx = (w + 7) // 8
    i0, r0 = (tile % tx) * 8, (tile // tx) * 8
    i1, r1 = min(i0 + 7, w - 1), min(r0 + 7, h - 1)
    top, one = (1 << 23) - 1, 1  # gen_range(-1, 1) = 2 k / 2^23 - 1 from draw k << 9: the largest and the smallest
    mid = 1 << 22                # value that the disk's rejection (x² + y² < 1) lets through beside a 0, and 0
    dg = lambda sgn: int(round((sgn * 0.70710 + 1.0) * 0.5 * 2 ** 23))
    lens = [(mid, mid), (top, mid), (one, mid), (mid, top), (mid, one), (dg(1), dg(1)), (dg(-1), dg(1)),
            (dg(1), dg(-1)), (dg(-1), dg(-1))]
    out, used = np.zeros(7, f32), C.c_uint32()
    O, D = [], []
    for i in (i0, i1):
        for r in (r0, r1):
            j = h - 1 - r
            for jx in (f32(0.0), f32(BELOW_ONE)):
                for jy in (f32(0.0), f32(BELOW_ONE)):
                    s = f32(f32(i) + jx) / f32(w - 1)
                    t = f32(f32(j) + jy) / f32(h - 1)
                    for kx, ky in lens:
                        draws = np.array([kx << 9, ky << 9, 0x80000000], np.uint32)
                        L.oracle_get_ray(C.byref(ocam), s, t, draws.ctypes.data_as(C.POINTER(C.c_uint32)), 3,
                                         orc.fp(out), C.byref(used))
                        assert used.value == 3, "a lens draw was rejected"
                        O.append(out[0:3].astype(np.float64))
                        D.append(out[3:6].astype(np.float64))
    return np.array(O), np.array(D)


def test_beam_never_rejects_a_box_on_an_f32_ray_at_large_magnitudes(rtw, orc):
    """The margins' own case (the f32 ray lies within 32 u M (1 + t) of the ideal one): rays as the f32
    arithmetic forms them from cameras at |coordinates| of 2^8 .. 2^14, and thin boxes (half extent 1e-3, 1e-5 or one
    ulp of the coordinate) around points of those rays at parameter 0.02, 0.5, 1, 3 and 50 (1 = the focus plane).  The
    truth is the exact slab test in double of the line through the f32 origin and direction.  A control set of equal
    boxes moved sideways, four times the beam's width and margin away, must be rejected at least one time in five:
    the test still culls at these magnitudes."""
    rng = np.random.default_rng(12)
    f32 = np.float32
    pairs = meeting = boxes = 0
    control = control_rejected = 0
    for ci, (cam, focus) in enumerate(_shifted_cameras(rtw)):
        w, h = FRAMES[ci % len(FRAMES)]
        cu, cv = (np.array(list(getattr(cam.c, k)), np.float64) for k in ("u", "v"))
        R = float(cam.c.lens_radius)
        M = max(abs(x) for k in ("origin", "lower_left_corner", "horizontal", "vertical") for x in getattr(cam.c, k))
        # the focus plane's extent per tile: 8 pixels of the image rectangle, across and up
        tile_f = 8.0 * max(np.linalg.norm(list(cam.c.horizontal)) / (w - 1), np.linalg.norm(list(cam.c.vertical)) / (h - 1))
        for tile in _tiles(w, h):
            O, D = _f32_tile_rays(orc, cam, w, h, tile)
            n_box = 80
            k = rng.integers(0, len(O), n_box)
            t = np.tile([0.02, 0.5, 1.0, 3.0, 50.0], n_box // 5)
            p = O[k] + t[:, None] * D[k]
            c = p.astype(f32)
            half = np.tile(np.repeat([1e-3, 1e-5, 0.0], 5), n_box // 15 + 1)[:n_box, None]
            # at least one ulp on each side: the box holds the double point whatever its centre rounded to
            lo = np.minimum((c - half).astype(f32), np.nextafter(c, f32(-np.inf)))
            hi = np.maximum((c + half).astype(f32), np.nextafter(c, f32(np.inf)))
            hit = _slab_hits(O, D, lo.astype(np.float64), hi.astype(np.float64))
            assert hit[np.arange(n_box), k].all(), "a box does not hold the point it was built around"
            for b in range(n_box):
                may = rtw.diag_tile_beam(cam, w, h, tile, lo[b], hi[b])
                boxes += 1
                pairs += hit.shape[1]
                meeting += int(hit[b].sum())
                q = np.flatnonzero(hit[b])[0]
                assert may, f"camera {ci} {w}x{h} tile {tile}: box {lo[b]}..{hi[b]} (parameter {t[b]}) rejected, " \
                            f"but the f32 ray {O[q]} + t {D[q]} meets it"
            # the control: the same boxes beside the beam, along the lens' u or v axis
            for b in range(0, n_box, 4):
                width = t[b] * tile_f + abs(1.0 - t[b]) * 2.0 * R + 2.5e-4 * (2.0 + t[b]) * M
                side = (cu if b % 8 else cv) * (4.0 * width + 1e-2) * (1 if b % 3 else -1)
                control += 1
                control_rejected += not rtw.diag_tile_beam(cam, w, h, tile, (lo[b] + side).astype(f32),
                                                           (hi[b] + side).astype(f32))
    assert boxes >= 10_000 and meeting >= 10_000, f"only {meeting} of {pairs} (ray, box) pairs intersect"
    assert control >= 2_000 and control_rejected * 5 >= control, \
        f"the beam test rejected {control_rejected} of {control} boxes beside the beam: it culls nothing"


def test_beam_on_the_preset_view(rtw):
    """The shape of the estimate the lists rest on: under the jumpy-balls camera at 1080p a 0.2 ball's box is a
    candidate of the tile it projects to and of few others."""
    cam = rtw.Camera.new((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 16 / 9, 0.1, 10.0)
    w, h = 1920, 1080
    lo, hi = np.float32([3.8, 0.0, 0.8]), np.float32([4.2, 0.4, 1.2])
    n = sum(rtw.diag_tile_beam(cam, w, h, t, lo, hi) for t in range(rtw.n_tiles(w, h)))
    assert 1 <= n <= 0.02 * rtw.n_tiles(w, h), n
