"""CPU: the forward camera's gather table (aido1_amd/camera.py) against the
per-pixel restatement of tests/ego_ref.py, its geometry, check_table, and the
oracle's line detector on gathered oracle frames (so that the GPU comparison of
tests/test_gpu_camera.py is not a comparison of empty masks)."""
import numpy as np
import pytest

import ego_ref as ER
from conftest import map_rows
from oracle import oracle_c as OC

from aido1_amd.camera import NONE, EgoCamera, check_table, resolve

CAMERAS = {
    'default': {},
    'distorted': dict(distortion=True),
    'other': dict(floor_dist=0.12, tilt_deg=25.0, fov_y_deg=60.0),
    'other-distorted': dict(floor_dist=0.09, tilt_deg=12.0, fov_y_deg=90.0, distortion=True,
                            k1=-0.25, k2=0.05),
}


@pytest.fixture(scope='module')
def tables():
    return {k: EgoCamera(**kw).table() for k, kw in CAMERAS.items()}


@pytest.mark.parametrize('name', sorted(CAMERAS))
def test_table_equals_the_restatement(tables, name):
    t = tables[name]
    assert t.dtype == np.uint16 and t.shape == (120, 160)
    want = ER.ego_table(**CAMERAS[name])
    assert np.array_equal(t, want), np.argwhere(t != want)[:4]
    check_table(t)
    assert (t != NONE).any()


@pytest.mark.parametrize('name,first,share', [('default', 40, 0.660), ('distorted', 41, 0.629)])
def test_default_tables_see_the_ground_below_the_horizon(tables, name, first, share):
    """Rows above the first ground row are sky; at least 60 % of the frame
    sees the raster (66.0 % / 62.9 %, to the figure's three digits)."""
    t = tables[name]
    assert (t[:first] == NONE).all()
    assert (t[first] != NONE).any()
    seen = (t != NONE).mean()
    assert seen >= 0.60
    assert abs(seen - share) < 5e-4, seen


def test_source_row_does_not_grow_up_the_frame(tables):
    """Without distortion a pixel higher in the frame looks at least as far:
    down every column the source row does not grow as the row index falls."""
    t = tables['default']
    for c in range(160):
        col = t[:, c]
        rows = [int(v) // 160 for v in col if v != NONE]   # top of the frame first
        assert rows == sorted(rows), c
        # and the column's ground pixels are one run that ends at the bottom row or where
        # the ray leaves the raster sideways
        idx = np.flatnonzero(col != NONE)
        assert len(idx) == 0 or (np.diff(idx) == 1).all(), c
    assert t[119, 80] // 160 > t[40, 80] // 160


def test_columns_mirror(tables):
    """Without distortion columns c and 159 - c show the same source row and
    mirrored source columns (cs and 159 - cs), wherever l / 0.01 is not an
    integer (there floor() breaks the symmetry)."""
    t = tables['default']
    checked = 0
    for r in range(120):
        for c in range(80):
            a, la = ER.ego_entry(r, c)
            b, lb = ER.ego_entry(r, 159 - c)
            if la is None or la == np.floor(la) or lb == np.floor(lb):
                continue
            assert (a == NONE) == (b == NONE), (r, c)
            assert t[r, c] == a and t[r, 159 - c] == b
            if a != NONE:
                assert a // 160 == b // 160 and a % 160 == 159 - b % 160, (r, c)
                checked += 1
    assert checked > 5000


def test_lateral_sign():
    """A marking left of centre in the top-down frame is left of centre in the
    forward frame: left columns gather from left source columns."""
    t = EgoCamera().table()
    left, right = t[:, :80], t[:, 80:]
    assert ((left[left != NONE] % 160) < 80).all()
    assert ((right[right != NONE] % 160) >= 80).all()


def test_check_table_refuses():
    t = EgoCamera().table()
    bad = t.copy()
    bad[7, 9] = 19200
    with pytest.raises(ValueError, match='19200'):
        check_table(bad)
    bad[7, 9] = 65534
    with pytest.raises(ValueError):
        check_table(bad)
    with pytest.raises(ValueError, match='shape'):
        check_table(t.reshape(-1))
    with pytest.raises(ValueError, match='shape'):
        check_table(t[:, :159])
    with pytest.raises(ValueError, match='uint16'):
        check_table(t.astype(np.int32))
    with pytest.raises(ValueError):
        check_table(t.tolist())
    edge = t.copy()
    edge[0, 0], edge[0, 1], edge[0, 2] = 0, 19199, NONE
    assert check_table(edge) is edge


def test_resolve():
    assert resolve(None) is None and resolve(None, distortion=True) is None
    assert not resolve('ego').distortion and resolve('ego', distortion=True).distortion
    cam = EgoCamera(tilt_deg=30.0)
    assert resolve(cam, distortion=True) is cam
    with pytest.raises(ValueError):
        resolve('fisheye')
    with pytest.raises(ValueError):
        EgoCamera(floor_dist=0.0)


@pytest.mark.parametrize('name', ['default', 'distorted'])
def test_forward_frames_carry_lines(tables, name):
    """loop_empty, seed 3, 64 reset poses: through each default table the
    oracle's line detector finds a white mask and edges in every frame and a
    yellow mask in at least 85 % of them."""
    rows = map_rows('loop_empty')
    ob = OC.OracleBatch(rows, 64, seed=3)
    ob.reset()
    s = ob.state()
    orend = OC.OracleRender(rows)
    _, _, rgb = orend.render(s['x'], s['z'], s['angle'])
    fwd = ER.gather(rgb, tables[name])
    assert not np.array_equal(fwd, rgb)
    masks = orend.line_detect(fwd[..., ::-1])
    assert (masks[:, 0] > 0).any((1, 2)).all()
    assert (masks[:, 3] > 0).any((1, 2)).all()
    assert (masks[:, 1] > 0).any((1, 2)).mean() >= 0.85
