"""The forward-camera observation's gather table (host only, float64).

The reference trains on the robot's forward camera (Simulator(camera_width=640,
camera_height=480, distortion=True), duckietown_rl/env.py:12-16, resized to
120x160).  This build renders a 120x160 top-down raster of the ground ahead of
the robot.  With the camera rigid on the robot and the ground flat, the forward
view of the ground is a fixed function of that raster: every pixel of the
forward frame looks at one raster pixel or at nothing (sky, or ground past the
raster's 1.2 m).  ``EgoCamera.table()`` is that function as a constant
uint16[120, 160] table; dt_render_camera (include/dtsim.h) uploads it and the
render kernel gathers the frame through it (phase 0d) before the line detector
runs.  Pinhole, tilt, field of view and lens distortion are only different
tables.

The view is build-defined, like the raster it is made from: 1 cm ground
resolution (so it is blocky near the camera), nothing beyond 1.2 m, and parity
with upstream's OpenGL frame is not pinned.
"""
import math

import numpy as np

H, W = 120, 160
NPIX = H * W
NONE = 0xFFFF          # a table entry that sees nothing
RES = 0.01             # metres per raster pixel


class EgoCamera:
    """A pinhole camera rigid on the robot, looking forward and down.

    The defaults are upstream gym-duckietown's constants as recalled (the
    package is absent): CAMERA_FLOOR_DIST 0.108 m, CAMERA_ANGLE 19.15 degrees
    of downward tilt, CAMERA_FOV_Y 75 degrees, and the fisheye model's first two
    radial coefficients k1, k2 of its distortion.  The distortion model here is
    radial only: upstream's tangential terms (p1, p2) and k3 are left out.

    floor_dist: height of the optical centre over the ground, metres.
    tilt_deg: downward tilt of the optical axis.
    fov_y_deg: vertical field of view of the 120-row frame.
    distortion: the frame is the distorted (fisheye) image: each pixel is
      undistorted (eight fixed-point iterations of the radial model) before its
      ray is cast.
    """

    def __init__(self, floor_dist=0.108, tilt_deg=19.15, fov_y_deg=75.0, distortion=False,
                 k1=-0.2944, k2=0.0701):
        self.floor_dist = float(floor_dist)
        self.tilt_deg = float(tilt_deg)
        self.fov_y_deg = float(fov_y_deg)
        self.distortion = bool(distortion)
        self.k1 = float(k1)
        self.k2 = float(k2)
        if not (self.floor_dist > 0.0 and 0.0 < self.fov_y_deg < 180.0 and
                -90.0 <= self.tilt_deg <= 90.0):
            raise ValueError('EgoCamera: floor_dist > 0, 0 < fov_y_deg < 180, |tilt_deg| <= 90')

    def __repr__(self):
        return 'EgoCamera(floor_dist=%r, tilt_deg=%r, fov_y_deg=%r, distortion=%r, k1=%r, k2=%r)' % (
            self.floor_dist, self.tilt_deg, self.fov_y_deg, self.distortion, self.k1, self.k2)

    def table(self):
        """uint16[120, 160]: entry [r, c] is the top-down raster's pixel
        rs * 160 + cs that the forward frame's pixel (r, c) shows, or 0xFFFF.

        The raster's origin is the camera's ground point (pose +
        camera_forward_dist * dir), its row 119 the nearest centimetre ahead and
        its columns grow to the robot's right, as the forward frame's do.  Every
        operation is float64 in this order (tests/ego_ref.py restates it a pixel
        at a time)."""
        f = 60 / math.tan(math.radians(self.fov_y_deg) / 2)
        tilt = math.radians(self.tilt_deg)
        st, ct = math.sin(tilt), math.cos(tilt)
        c = np.arange(W, dtype=np.float64).reshape(1, W)
        r = np.arange(H, dtype=np.float64).reshape(H, 1)
        ud = np.broadcast_to((c + 0.5 - 80) / f, (H, W))
        vd = np.broadcast_to((r + 0.5 - 60) / f, (H, W))
        u, v = ud, vd
        if self.distortion:
            for _ in range(8):
                r2 = u * u + v * v
                s = 1 + self.k1 * r2 + self.k2 * r2 * r2
                u = ud / s
                v = vd / s
        down = st + v * ct
        fwd = ct - v * st
        ok = down > 0
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            t = self.floor_dist / np.where(ok, down, 1.0)
            d = t * fwd
            l = t * u   # noqa: E741
            ok &= ~(d < 0)
            rs = 119 - np.floor(d / RES)
            cs = np.floor(l / RES + 80.0)
            ok &= (rs >= 0) & (rs <= H - 1) & (cs >= 0) & (cs <= W - 1)
        src = np.where(ok, rs, 0.0).astype(np.int64) * W + np.where(ok, cs, 0.0).astype(np.int64)
        return np.where(ok, src, NONE).astype(np.uint16)


def check_table(t):
    """Raise ValueError unless t is a uint16 [120, 160] array whose entries are
    raster pixels (0..19199) or 0xFFFF: what dt_render_camera accepts."""
    if not isinstance(t, np.ndarray) or t.dtype != np.uint16:
        raise ValueError('camera table: a numpy uint16 array expected, got %s'
                         % (getattr(t, 'dtype', type(t).__name__),))
    if t.shape != (H, W):
        raise ValueError('camera table: shape (120, 160) expected, got %s' % (t.shape,))
    bad = (t >= NPIX) & (t != NONE)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise ValueError('camera table: entry [%d, %d] = %d is neither a pixel (0..19199) nor '
                         '65535' % (r, c, int(t[r, c])))
    return t


def resolve(camera, distortion=False):
    """The EgoCamera of a `camera=` argument: None (top-down), 'ego' (the
    defaults; with `distortion`, the distorted frame) or an EgoCamera."""
    if camera is None:
        return None
    if isinstance(camera, EgoCamera):
        return camera
    if camera == 'ego':
        return EgoCamera(distortion=bool(distortion))
    raise ValueError("camera must be None, 'ego' or an EgoCamera, not %r" % (camera,))
