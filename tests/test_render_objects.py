"""Objects in the observation, the parts that need no GPU: the map's footprint
records (TileMap.render_table) and the restatement the GPU tests compare with
(tests/render_objects_ref.py)."""
import ctypes
import math

import numpy as np

import render_objects_ref as RO
from aido1_amd.maps import load_map


def test_render_table_of_loop_obstacles():
    m = load_map('loop_obstacles')
    t = m.render_table
    assert t.shape == (5, 8) and t.dtype == np.float32
    assert len(t) == len(m.spawn_table)          # every object, collidable or not
    assert [o.kind for o in m.objects] == ['duckie', 'cone', 'barrier', 'tree', 'house']
    assert not m.objects[3].collidable           # the tree is drawn all the same
    for q, o in zip(t.astype(np.float64), m.objects):
        c = o.corners
        got = np.array([q[0:2], q[0:2] + q[2:4], q[0:2] + q[2:4] + q[4:6], q[0:2] + q[4:6]])
        # one float32 rounding a term, of values up to ~2.3 m
        assert np.abs(got - c).max() <= 3 * 2.3 * 2.0 ** -24
        e1, e2 = c[1] - c[0], c[3] - c[0]
        assert q[6] == np.float32(e1 @ e1) and q[7] == np.float32(e2 @ e2)
        assert abs(e1 @ e2) <= 1e-12               # a rectangle


def test_map_without_objects_has_an_empty_table():
    t = load_map('loop_empty').render_table
    assert t.shape == (0, 8) and t.dtype == np.float32


def test_red_grey_is_the_palette_entry():
    """An object pixel's grey, float64 rgb2gray of (220, 30, 30) rounded to
    float32, is entry 3 of the library's palette grey table."""
    from aido1_amd import _lib
    buf = (ctypes.c_float * 8)()
    assert _lib.lib().dt_palette_gray(buf) == 0
    want = np.float32(0.2125 * (220 / 255.0) + 0.7154 * (30 / 255.0) + 0.0721 * (30 / 255.0))
    assert RO.RED_GRAY == np.float32(buf[RO.PAL_RED])
    assert abs(float(want) - float(RO.RED_GRAY)) <= 2.0 ** -24


def test_axis_aligned_objects_fill_their_pixel_rectangle():
    """The cone and the tree (rotate 0) seen by a camera looking along +x: rows
    run down -x and columns along +z, so the footprint is the rectangle of the
    pixel centres inside [x0, x1] x [z0, z1].  The camera is placed so that no
    pixel centre lies within 0.25 px of a side, far above float32 rounding."""
    m = load_map('loop_obstacles')
    t = m.render_table
    for k in (1, 3):
        o = m.objects[k]
        assert o.rotate == 0.0
        (x0, z0), (x1, z1) = o.corners.min(0), o.corners.max(0)
        # camera centre: x0 at row coordinate 59.35, z0 at column coordinate 70.35
        cam_x, cam_z = x0 - 0.6015, z0 + 0.0915
        rows = 119.5 - (np.array([x0, x1]) - cam_x) * 100.0     # row coordinate of each side
        cols = 79.5 + (np.array([z0, z1]) - cam_z) * 100.0
        for v in np.r_[rows, cols]:
            assert 0.25 <= v - math.floor(v) <= 0.75, v
        want = np.zeros((RO.H, RO.W), bool)
        want[math.ceil(rows[1]):math.floor(rows[0]) + 1,
             math.ceil(cols[0]):math.floor(cols[1]) + 1] = True
        assert want.sum() == round((x1 - x0) * 100) * round((z1 - z0) * 100)
        got = RO.object_mask(t[k:k + 1], cam_x - RO.CAM_FWD, cam_z, 0.0)[0]
        assert np.array_equal(got, want)


def test_box_culling_never_changes_a_pixel():
    """What the kernel relies on: testing only the pixels of each object's
    projected box, 2 px wider, sets exactly the pixels the test of every pixel
    sets -- on 200 random poses around the objects, with objects clipped at
    every frame edge and poses that see none."""
    m = load_map('loop_obstacles')
    t = m.render_table
    rng = np.random.default_rng(11)
    centres = [o.corners.mean(0) for o in m.objects]
    x, z, a = RO.place_poses(centres, rng, 200, ahead=(-0.2, 1.4), lateral=1.0)
    full = RO.object_mask(t, x, z, a)
    assert np.array_equal(RO.object_mask(t, x, z, a, cull_margin=2.0), full)
    per_frame = full.reshape(200, -1).sum(1)
    assert (per_frame > 0).mean() >= 0.5 and (per_frame == 0).any()
    for edge in (full[:, 0], full[:, -1], full[:, :, 0], full[:, :, -1]):
        assert edge.any()
