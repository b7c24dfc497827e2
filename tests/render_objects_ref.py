"""CPU restatement of the render's object phase (dt_render_objects,
include/dtsim.h) in numpy float32, and the frame the renderer must produce
with it: the C oracle's object-free frame with the footprints painted red.

A pixel (row r, column c) belongs to an object with record q iff

    f  = (119.5f - r) * 0.01f;  l = (c - 79.5f) * 0.01f
    wx = (V.cx + f*V.dirx) + l*V.rx;   wz = (V.cz + f*V.dirz) + l*V.rz
    dx = wx - q0;  dz = wz - q1
    s  = dx*q2 + dz*q3;   t = dx*q4 + dz*q5
    inside = s >= 0 && s <= q6 && t >= 0 && t <= q7

every operation rounded to float32 (numpy float32 arrays never contract), V
the float32 camera oracle/render_oracle.c builds from the float64 pose.
"""
import math

import numpy as np

H, W = 120, 160
RED = (220, 30, 30)      # palette byte 3
PAL_RED = 3
F = np.float32
# PreliminaryTransformer's rgb2gray of RED in float64, rounded once
RED_GRAY = F((220 * (1.0 / 255.0) * 0.2125 + 30 * (1.0 / 255.0) * 0.7154)
             + 30 * (1.0 / 255.0) * 0.0721)
CAM_FWD = 0.066          # EnvConfig.camera_forward_dist (CAMERA_FORWARD_DIST)


def camera(x, z, angle, cam_fwd=CAM_FWD):
    """The float32 camera of each pose, as arrays [n, 1, 1]."""
    x, z, angle = (np.atleast_1d(np.asarray(v, np.float64)) for v in (x, z, angle))
    c, s = np.cos(angle), np.sin(angle)
    v = dict(cx=(x + cam_fwd * c).astype(F), cz=(z + cam_fwd * (-s)).astype(F),
             dirx=c.astype(F), dirz=-(s.astype(F)), rx=s.astype(F), rz=c.astype(F))
    return {k: a[:, None, None] for k, a in v.items()}


def object_boxes(q, V, margin):
    """The kernel's cull: per pose the pixel box (r0, r1, c0, c1, inclusive,
    clamped to the frame) of the record's four projected corners, `margin`
    pixels wider, and whether it meets the frame.  Arrays [n]."""
    q = np.asarray(q, F)
    zero = F(0.0)
    cs, rs = [], []
    for k in range(4):   # c0, c0 + e1, c0 + e1 + e2, c0 + e2
        px = (q[0] + (q[2] if k in (1, 2) else zero)) + (q[4] if k >= 2 else zero)
        pz = (q[1] + (q[3] if k in (1, 2) else zero)) + (q[5] if k >= 2 else zero)
        ax, az = px - V['cx'][:, 0, 0], pz - V['cz'][:, 0, 0]
        fa = ax * V['dirx'][:, 0, 0] + az * V['dirz'][:, 0, 0]
        la = ax * V['rx'][:, 0, 0] + az * V['rz'][:, 0, 0]
        cs.append(la * F(100.0) + F(79.5))
        rs.append(F(119.5) - fa * F(100.0))
    m = F(margin)
    cmin, cmax = np.floor(np.min(cs, 0) - m), np.ceil(np.max(cs, 0) + m)
    rmin, rmax = np.floor(np.min(rs, 0) - m), np.ceil(np.max(rs, 0) + m)
    vis = (cmax >= 0) & (cmin <= W - 1) & (rmax >= 0) & (rmin <= H - 1)
    return (np.maximum(rmin, 0), np.minimum(rmax, H - 1), np.maximum(cmin, 0),
            np.minimum(cmax, W - 1), vis)


def object_mask(table, x, z, angle, cam_fwd=CAM_FWD, cull_margin=None):
    """bool [n, 120, 160]: the pixels some object of `table` ([M, 8] float32
    records) covers at each pose.  cull_margin: None tests every pixel against
    every object; a number of pixels tests only the pixels of each object's
    box (object_boxes), as the kernel does."""
    table = np.asarray(table, F).reshape(-1, 8)
    V = camera(x, z, angle, cam_fwd)
    n = len(V['cx'])
    r = np.arange(H, dtype=F)[None, :, None]
    c = np.arange(W, dtype=F)[None, None, :]
    f = (F(119.5) - r) * F(0.01)
    lat = (c - F(79.5)) * F(0.01)
    wx = (V['cx'] + f * V['dirx']) + lat * V['rx']
    wz = (V['cz'] + f * V['dirz']) + lat * V['rz']
    assert wx.dtype == F and wz.dtype == F
    out = np.zeros((n, H, W), bool)
    for q in table:
        dx, dz = wx - q[0], wz - q[1]
        s = dx * q[2] + dz * q[3]
        t = dx * q[4] + dz * q[5]
        assert s.dtype == F and t.dtype == F
        inside = (s >= 0) & (s <= q[6]) & (t >= 0) & (t <= q[7])
        if cull_margin is not None:
            r0, r1, c0, c1, vis = object_boxes(q, V, cull_margin)
            k = lambda a: a[:, None, None]   # noqa: E731
            inside &= k(vis) & (r >= k(r0)) & (r <= k(r1)) & (c >= k(c0)) & (c <= k(c1))
        out |= inside
    return out


def compose(orend, table, x, z, angle):
    """The expected frame: (grey [n,120,160] f32, masks [n,4,120,160] u8, rgb
    [n,120,160,3] u8, object mask [n,120,160] bool).  orend: an
    oracle_c.OracleRender of the map (its line parameters are the masks')."""
    gray, _, rgb = orend.render(x, z, angle)
    obj = object_mask(table, x, z, angle, orend.cfg.camera_forward_dist)
    rgb = rgb.copy()
    rgb[obj] = RED
    masks = orend.line_detect(rgb[..., ::-1])
    gray = gray.copy()
    gray[obj] = RED_GRAY
    return gray, masks, rgb, obj


def place_poses(centres, rng, n, ahead=(0.15, 1.1), lateral=0.7, cam_fwd=CAM_FWD):
    """n poses (x, z, angle), pose i looking at object i % len(centres) from a
    random direction so that its centre sits ahead[0]..ahead[1] m in front of
    the camera and within +-lateral m to its side (the frame shows 0..1.2 m
    ahead, +-0.8 m to the side)."""
    x, z, a = np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(n):
        px, pz = centres[i % len(centres)]
        a[i] = rng.uniform(-math.pi, math.pi)
        x[i], z[i] = pose_seeing(px, pz, a[i], rng.uniform(*ahead),
                                 rng.uniform(-lateral, lateral), cam_fwd)
    return x, z, a


def pose_seeing(px, pz, angle, ahead, lat, cam_fwd=CAM_FWD):
    """The pose (x, z) at `angle` whose camera has world point (px, pz) `ahead`
    m in front and `lat` m to the right."""
    dx, dz = math.cos(angle), -math.sin(angle)
    rx, rz = math.sin(angle), math.cos(angle)
    return (px - (ahead + cam_fwd) * dx - lat * rx, pz - (ahead + cam_fwd) * dz - lat * rz)
