// rtw_tile_beam.h — can a camera ray of one 8x8 tile meet a box?  The conservative test behind the per-tile
// primitive lists ("Camera rays against per-tile lists"), shared by the gfx950 list builder
// (rtw_kernel.hip tile_list_kernel) and the host (rtw_diag_tile_beam, tests/test_tile_beam.py).
//
// A camera ray (camera.rs:66-74) is A + t (F - A), t >= 0, with A = origin + a u + b v on the lens, (a, b) in the
// square [-R, R]² that bounds the lens disk, and F = llc + su horizontal + sv vertical on the focus plane, (su, sv) in
// the tile's range.  In any orthonormal frame (x, y, z) every coordinate of A and of F lies in an interval (a sum of
// products of intervals), and the ray's point at parameter t has coordinate c in
//   [t f0 + min((1-t) a0, (1-t) a1),  t f1 + max((1-t) a0, (1-t) a1)]      (A_c in [a0, a1], F_c in [f0, f1]).
// The frame's z points from the lens to the tile range's middle; when the whole F interval lies in front of the whole A
// interval on z (else the test answers "may hit") both z bounds grow with t, so the parameters at which the ray can be
// inside the box's z range form one interval [t0, t1].  The upper bound of x (and y) is convex in t and the lower one
// concave: over [t0, t1] their extremes sit at t0 and t1, and the box is rejected when on x or on y it lies wholly
// above the larger upper bound or wholly below the smaller lower bound.  Nothing here assumes that the camera's vectors
// are orthogonal or that u, v are parallel to horizontal, vertical: a skewed camera only widens the intervals.
//
// Everything is evaluated in double on f32 inputs.  Margins (DESIGN.md §2 derives the bound they are measured
// against): the (su, sv) range is widened by 1e-3 pixel + 1e-5 relative, the box inflated by
// BEAM_MARGIN (2 + t1) x the largest magnitude among the camera's terms and the box's corners, and [t0, t1] by 1e-9
// relative + 1e-12.  Every comparison rejects; a NaN rejects nothing.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RTW_BEAM_HD __host__ __device__ __forceinline__
#else
#define RTW_BEAM_HD static inline
#endif

namespace rtw {

// 131 x 32 u (u = 2^-24): DESIGN.md §2 bounds the f32 ray's distance from the ideal beam at parameter t by
// 32 u (1 + t) x the largest magnitude
constexpr double BEAM_MARGIN = 2.5e-4;

// The camera's part of the test (once per render call): the frame, the lens' interval per axis, and what a tile's
// F interval is assembled from.
struct BeamCamera {
  double ex[3], ey[3], ez[3];  // the orthonormal frame; coordinates are relative to the camera's origin
  double a[3];                 // |A_c| <= a[c]: the lens square's half extent on each axis
  double l[3], hz[3], vt[3];   // llc - origin, horizontal, vertical in the frame
  double mag;                  // the largest magnitude among the camera's terms (absolute coordinates)
  double org[3];               // the camera's origin
  bool ok;                     // the frame exists (a finite, non-degenerate camera)
};

RTW_BEAM_HD double beam_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

RTW_BEAM_HD BeamCamera beam_camera(const float origin[3], const float u[3], const float v[3], const float llc[3],
                                   const float horizontal[3], const float vertical[3], float lens_radius) {
  BeamCamera c;
  double o[3], lu[3], lv[3], ll[3], hh[3], vv[3], z[3], x[3];
  for (int k = 0; k < 3; ++k) {
    o[k] = origin[k]; lu[k] = u[k]; lv[k] = v[k]; hh[k] = horizontal[k]; vv[k] = vertical[k];
    ll[k] = (double)llc[k] - o[k];
    c.org[k] = o[k];
  }
  // z: from the lens to the middle of the focus plane's image rectangle
  for (int k = 0; k < 3; ++k) z[k] = ll[k] + 0.5 * hh[k] + 0.5 * vv[k];
  const double zn = sqrt(beam_dot(z, z));
  for (int k = 0; k < 3; ++k) c.ez[k] = z[k] / zn;
  // x: horizontal's part across z
  const double hz = beam_dot(hh, c.ez);
  for (int k = 0; k < 3; ++k) x[k] = hh[k] - hz * c.ez[k];
  const double xn = sqrt(beam_dot(x, x));
  for (int k = 0; k < 3; ++k) c.ex[k] = x[k] / xn;
  c.ey[0] = c.ez[1] * c.ex[2] - c.ez[2] * c.ex[1];
  c.ey[1] = c.ez[2] * c.ex[0] - c.ez[0] * c.ex[2];
  c.ey[2] = c.ez[0] * c.ex[1] - c.ez[1] * c.ex[0];
  const double R = fabs((double)lens_radius);
  const double* E[3] = {c.ex, c.ey, c.ez};
  double m = R;
  for (int k = 0; k < 3; ++k) {
    c.a[k] = R * (fabs(beam_dot(lu, E[k])) + fabs(beam_dot(lv, E[k])));
    c.l[k] = beam_dot(ll, E[k]);
    c.hz[k] = beam_dot(hh, E[k]);
    c.vt[k] = beam_dot(vv, E[k]);
    m = fmax(m, fmax(fabs(o[k]), fmax(fabs((double)llc[k]), fmax(fabs(hh[k]), fabs(vv[k])))));
  }
  c.mag = m;
  c.ok = zn > 0.0 && xn > 0.0 && zn < INFINITY && xn < INFINITY && m < INFINITY;
  return c;
}

// One tile's part: the F interval per axis and the reciprocals of the z slopes.
struct BeamTile {
  double f0[3], f1[3];
  double r11, r10, r00, r01;  // 1 / (fz1 - az1), 1 / (fz1 - az0), 1 / (fz0 - az0), 1 / (fz0 - az1)
  bool ok;                    // the focus interval lies in front of the lens interval on z
};

RTW_BEAM_HD BeamTile beam_tile(const BeamCamera& c, uint32_t w, uint32_t h, uint32_t tile) {
  BeamTile t;
  const uint32_t tiles_x = (w + 7u) / 8u;
  const uint32_t tx = tile % tiles_x, ty = tile / tiles_x;
  // pixel columns 8 tx .. 8 tx + 7 (+ [0, 1) jitter); rows 8 ty .. 8 ty + 7 are j = h - 1 - row (lib.rs:84-85).
  // A partial tile keeps the whole range: a superset.
  const double i0 = 8.0 * tx, i1 = i0 + 8.0;
  const double j1 = (double)h - 8.0 * ty, j0 = j1 - 8.0;
  const double pw = 1.0e-3 + 1.0e-5 * i1, ph = 1.0e-3 + 1.0e-5 * fabs(j1);
  const double su0 = (i0 - pw) / ((double)w - 1.0), su1 = (i1 + pw) / ((double)w - 1.0);
  const double sv0 = (j0 - ph) / ((double)h - 1.0), sv1 = (j1 + ph) / ((double)h - 1.0);
  for (int k = 0; k < 3; ++k) {
    const double h0 = c.hz[k] * su0, h1 = c.hz[k] * su1, v0 = c.vt[k] * sv0, v1 = c.vt[k] * sv1;
    t.f0[k] = c.l[k] + fmin(h0, h1) + fmin(v0, v1);
    t.f1[k] = c.l[k] + fmax(h0, h1) + fmax(v0, v1);
  }
  const double az = c.a[2];
  t.ok = c.ok && t.f0[2] - az > 1.0e-9 * (fabs(t.f0[2]) + az);
  t.r11 = 1.0 / (t.f1[2] - az);
  t.r10 = 1.0 / (t.f1[2] + az);
  t.r00 = 1.0 / (t.f0[2] + az);
  t.r01 = 1.0 / (t.f0[2] - az);
  return t;
}

// A world box in the camera's frame: the bounding box of its eight corners, and its largest |coordinate|.
struct BeamBox {
  double lo[3], hi[3], mag;
};
RTW_BEAM_HD BeamBox beam_box(const BeamCamera& c, const float lo[3], const float hi[3]) {
  BeamBox b;
  const double* E[3] = {c.ex, c.ey, c.ez};
  b.mag = 0.0;
  for (int k = 0; k < 3; ++k) b.mag = fmax(b.mag, fmax(fabs((double)lo[k]), fabs((double)hi[k])));
  for (int k = 0; k < 3; ++k) {
    // the extent of the box on axis E[k]: centre +- sum |half_j E[k][j]|
    double mid = 0.0, ext = 0.0;
    for (int j = 0; j < 3; ++j) {
      const double cj = 0.5 * ((double)lo[j] + (double)hi[j]) - c.org[j], hj = 0.5 * ((double)hi[j] - (double)lo[j]);
      mid += cj * E[k][j];
      ext += fabs(hj * E[k][j]);
    }
    b.lo[k] = mid - ext;
    b.hi[k] = mid + ext;
  }
  return b;
}

// the bounds of coordinate k of the beam at parameter t
RTW_BEAM_HD double beam_hi(const BeamCamera& c, const BeamTile& T, int k, double t) {
  return t * T.f1[k] + fabs(1.0 - t) * c.a[k];
}
RTW_BEAM_HD double beam_lo(const BeamCamera& c, const BeamTile& T, int k, double t) {
  return t * T.f0[k] - fabs(1.0 - t) * c.a[k];
}

// false only if no camera ray of the tile can meet the box
RTW_BEAM_HD bool beam_may_hit(const BeamCamera& c, const BeamTile& T, const BeamBox& b) {
  if (!T.ok) return true;
  const double az = c.a[2];
  const double mag = fmax(c.mag, b.mag);
  // the z range first with the margin of t = 0 .. 1, to bound t1; then with the margin of that t1
  double m = BEAM_MARGIN * 2.0 * mag;
  double t1 = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    const double z1 = b.hi[2] + m;
    if (z1 < -az) return false;  // wholly behind the lens
    // lo_z(t) = t fz0 - |1 - t| az <= z1: up to t = 1 the slope is fz0 + az, beyond it fz0 - az
    t1 = (z1 + az) * T.r00;
    if (t1 > 1.0) t1 = (z1 - az) * T.r01;
    t1 = t1 * (1.0 + 1.0e-9) + 1.0e-12;
    if (pass == 0) m = BEAM_MARGIN * (2.0 + t1) * mag;
  }
  // hi_z(t) = t fz1 + |1 - t| az >= z0: up to t = 1 the slope is fz1 - az, beyond it fz1 + az
  const double z0 = b.lo[2] - m;
  double t0 = 0.0;
  if (z0 > az) {
    t0 = (z0 - az) * T.r11;
    if (t0 > 1.0) t0 = (z0 + az) * T.r10;
    t0 = t0 * (1.0 - 1.0e-9) - 1.0e-12;
    if (t0 < 0.0) t0 = 0.0;
  }
  if (t0 > t1) return false;
  for (int k = 0; k < 2; ++k) {
    const double up = fmax(beam_hi(c, T, k, t0), beam_hi(c, T, k, t1));
    const double dn = fmin(beam_lo(c, T, k, t0), beam_lo(c, T, k, t1));
    if (b.lo[k] - m > up) return false;
    if (b.hi[k] + m < dn) return false;
  }
  return true;
}

}  // namespace rtw
