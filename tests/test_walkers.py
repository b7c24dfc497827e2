"""Walkers on the CPU: the map loader's tables, walker_index, and analytic cases
on the restatement the GPU tests compare against (tests/walkers_ref.py)."""
import math

import numpy as np
import pytest

import walkers_ref as WR
from conftest import map_objects, map_rows
from oracle import dtsim_ref as R


def load(name, **kw):
    from aido1_amd.maps import load_map
    return load_map(name, **kw)


def custom(tmp_path, objects):
    return load(WR.write_map(tmp_path / 'm.yaml', objects))


# ---- the loader ---------------------------------------------------------------------------
def test_loop_pedestrians_tables():
    m = load('loop_pedestrians')
    kinds = [(o.kind, o.static) for o in m.objects]
    assert kinds == [('duckie', False), ('duckie', False), ('cone', True)]
    assert m.has_walkers
    # object_table: the static collidables in load order, then the walkers in load order
    ot, wt = m.object_table, m.walker_table
    assert ot.shape == (3, 20) and wt.shape == (3, 5) and wt.dtype == np.float64
    assert np.array_equal(ot[0, :3], m.objects[2].pos)
    assert np.array_equal(ot[1, :3], m.objects[0].pos)
    assert np.array_equal(ot[2, :3], m.objects[1].pos)
    assert np.array_equal(wt[0], np.zeros(5))
    # upstream's defaults: 8 s at 30 Hz, 0.61 + 0.25 m at 0.02 m a step (0.88 > 0.86)
    for row, o in ((1, m.objects[0]), (2, m.objects[1])):
        a = math.radians(o.rotate)
        assert np.array_equal(wt[row], [math.cos(a), -math.sin(a), 0.02, 240.0, 44.0])
        assert (o.W, o.K, o.vel, o.wait, o.walk_distance) == (240, 44, 0.02, 8.0, 0.61)
    assert 43 * 0.02 <= 0.61 + 0.25 < 44 * 0.02
    # spawn_table and render_table keep plain load order, the walkers at home
    assert np.array_equal(m.spawn_table[:, :3], np.array([o.pos for o in m.objects]))
    assert np.array_equal(m.render_table[:, :2],
                          np.array([o.corners[0] for o in m.objects]).astype(np.float32))
    rw = m.render_walker_table
    assert rw.shape == (3, 4) and rw.dtype == np.float32
    for row, o in enumerate(m.objects[:2]):
        hx, hz = o.heading
        assert np.array_equal(rw[row], np.array([0.02 * hx, 0.02 * hz, 240, 44], np.float32))
    assert np.array_equal(rw[2], np.zeros(4, np.float32))
    # both walkers cross a straight: half way they stand on it
    for o in m.objects[:2]:
        hx, hz = o.heading
        mid = o.pos + 22 * 0.02 * np.array([hx, 0.0, hz])
        i, j = int(mid[0] // 0.61), int(mid[2] // 0.61)
        assert m.rows[j][i].startswith('straight')


def test_key_overrides(tmp_path):
    m = custom(tmp_path, WR.FIXTURE_OBJECTS)
    w1, w2, cone, w3 = m.objects
    assert (w1.W, w1.K, w1.vel) == (3, 44, 0.02)
    assert (w2.W, w2.K, w2.vel) == (6, 29, 0.03)          # 29 * 0.03 = 0.87 > 0.86
    assert (w3.W, w3.K, w3.walk_distance) == (0, 33, 0.4)  # 33 * 0.02 = 0.66 > 0.65
    assert cone.static and (cone.W, cone.K, cone.vel) == (0, 0, 0.0)
    # the restatement derives the same steps on its own
    ref = WR.WalkerSimRef(WR.FIXTURE_TILES, objects=WR.FIXTURE_OBJECTS)
    assert [(w.W, w.K) for w in ref.walkers] == [(3, 44), (6, 29), (0, 33)]
    # frame_rate scales W only
    m60 = load(WR.write_map(tmp_path / 'n.yaml'), frame_rate=60)
    assert [o.W for o in m60.objects] == [6, 12, 0, 0]
    # table order: cone (static) first, then the three walkers
    assert np.array_equal(m.object_table[:, :3], np.array([o.pos for o in (cone, w1, w2, w3)]))
    assert np.array_equal(m.walker_table[:, 3:], [[0, 0], [3, 44], [6, 29], [0, 33]])
    # the home records are the restatement's
    for row, w in zip(m.object_table[1:], ref.walkers):
        assert np.array_equal(row[4:12], w.corners.reshape(-1))
        assert np.array_equal(row[12:16], w.norm.reshape(-1))
        assert row[3] == w.safety_radius


def test_other_dynamic_kinds_are_still_refused(tmp_path):
    bot = dict(kind='duckiebot', pos=[1.5, 0.3], height=0.12, static=False,
               mesh_min=[-0.6, 0, -0.45], mesh_max=[0.6, 1, 0.45])
    with pytest.raises(NotImplementedError):
        custom(tmp_path, [bot])
    with pytest.raises(NotImplementedError):
        custom(tmp_path, [dict(bot, kind='cone')])
    with pytest.raises(ValueError):
        custom(tmp_path, [dict(WR.DUCKIE, pos=[1.5, 0.3], static=False, vel=0.0)])


def test_walker_off_the_road_is_collidable(tmp_path):
    on_grass = dict(WR.DUCKIE, pos=[1.5, 1.5])
    m = custom(tmp_path, [on_grass, dict(on_grass, static=False)])
    assert [o.collidable for o in m.objects] == [False, True]
    assert m.object_table.shape == (1, 20) and m.walker_table[0, 4] >= 1


def test_static_maps_are_unchanged():
    m = load('loop_obstacles')
    assert not m.has_walkers
    assert np.array_equal(m.walker_table, np.zeros((len(m.object_table), 5)))
    assert np.array_equal(m.render_walker_table, np.zeros((len(m.render_table), 4), np.float32))
    # object_table is what the oracle's MapRef collects, in its order
    ref = R.MapRef(map_rows('loop_obstacles'), objects=map_objects('loop_obstacles'))
    assert np.array_equal(m.object_table[:, :3], ref.collidable_centers)
    assert np.array_equal(m.object_table[:, 4:12],
                          np.array(ref.collidable_corners).reshape(-1, 8))
    for name in ('loop_empty', 'small_loop'):
        assert load(name).walker_table.shape == (0, 5)


# ---- walker_index --------------------------------------------------------------------------
@pytest.mark.parametrize('W,K', [(0, 1), (3, 7), (240, 44)])
def test_walker_index_against_a_step_by_step_loop(W, K):
    from aido1_amd.maps import walker_index
    period = 2 * (W + K)
    idx, direction, waited = 0, 1, 0
    seen = []
    for t in range(3 * period + 1):
        assert walker_index(t, W, K) == idx == WR.index_at(t, W, K), t
        seen.append(idx)
        if waited < W:
            waited += 1
            continue
        idx += direction
        if idx == (K if direction > 0 else 0):
            direction, waited = -direction, 0
    assert max(seen) == K and min(seen) == 0 and seen[period] == 0
    assert seen[W + K] == K and seen[:W + 1] == [0] * (W + 1)
    assert WR.index_by_stepping(period + W + 1, W, K) == (1 if K > 1 else K)


# ---- analytic cases on the restatement -------------------------------------------------------
OFF = R.CAMERA_FORWARD_DIST - R.ROBOT_LENGTH / 2


@pytest.fixture(scope='module')
def sim():
    return WR.WalkerSimRef(WR.FIXTURE_TILES, objects=WR.FIXTURE_OBJECTS)


def park(centre_x, centre_z):
    """cur_pos of an agent at angle 0 whose actual centre is (centre_x, centre_z)."""
    return np.array([centre_x - OFF, 0.0, centre_z])


def test_parked_agent_is_hit_when_the_walker_arrives(sim):
    """Walker 1 walks +z from z0 = 0.05 * 0.61 with half length 0.04 (its box
    0.08 x 0.064, turned by -90 degrees); the agent's box spans z 0.3 +- 0.075 in
    its path.  They touch from idx = ceil((0.225 - 0.04 - z0) / 0.02) = 8 until
    the walker's back edge is past 0.375: idx = 20.  W = 3, K = 44."""
    w = sim.walkers[0]
    assert (w.hx, w.hz) == (math.cos(math.radians(-90)), 1.0) and abs(w.hx) < 1e-15
    z0 = 0.05 * 0.61
    first = math.ceil((0.3 - 0.075 - 0.04 - z0) / 0.02)
    clear = math.floor((0.3 + 0.075 + 0.04 - z0) / 0.02) + 1
    assert (first, clear) == (8, 20)
    pos = park(1.5 * 0.61, 0.3)
    P = w.W + w.K
    for t in range(2 * P + 1):
        sim.place(t)
        idx = WR.index_at(t, w.W, w.K)
        assert sim._valid_pose(pos, 0.0) == (not first <= idx < clear), (t, idx)
    # in time: valid while t <= W (and until the walker arrives), hit at W + 8,
    # clear again at W + 20, hit again on the way back
    valid = []
    for t in range(2 * P):
        sim.place(t)
        valid.append(sim._valid_pose(pos, 0.0))
    assert all(valid[:w.W + first]) and not any(valid[w.W + first:w.W + clear])
    assert all(valid[w.W + clear:P + w.W + (w.K - clear) + 1])
    assert not valid[P + w.W + (w.K - clear) + 1]
    sim.place(0)


def test_penalty_turns_negative_at_the_computed_distance(sim):
    """The safety circles (0.162 and 1.8 * hypot(0.5, 0.4) * 0.08) meet when the
    centres are closer than their sum: walker 1, 0.2695 m from the parked agent
    at home, is within it from idx = 1 on."""
    w = sim.walkers[0]
    reach = R.AGENT_SAFETY_RAD + w.safety_radius
    assert w.safety_radius == 1.8 * (np.hypot(0.5, 0.4) * 0.08)
    d0 = 0.3 - 0.05 * 0.61
    first = math.floor((d0 - reach) / 0.02) + 1
    assert first == 1
    pos = park(1.5 * 0.61, 0.3)
    for t in range(0, w.W + 6):
        sim.place(t)
        pen = sim.proximity_penalty2(pos, 0.0)
        idx = WR.index_at(t, w.W, w.K)
        if idx < first:
            assert pen == 0
        else:
            assert pen == pytest.approx((d0 - 0.02 * idx) - reach, abs=1e-12) and pen < 0
    sim.place(0)


def test_reset_puts_the_walkers_home():
    s = WR.WalkerSimRef(WR.FIXTURE_TILES, seed=5, objects=WR.FIXTURE_OBJECTS)
    s.reset()
    for t in range(1, 31):
        s.update_physics(np.array([0.0, 0.0]))
        assert s.step_count == t
    moved = [not np.array_equal(s.map.collidable_corners[s.first + j], w.corners)
             for j, w in enumerate(s.walkers)]
    assert moved == [True, True, True]
    c = s.map.collidable_corners[s.first]
    assert np.array_equal(c, s.walkers[0].corners + np.array(s.walkers[0].shift(30)))
    s.reset()
    assert s.step_count == 0
    for j, w in enumerate(s.walkers):
        assert np.array_equal(s.map.collidable_corners[s.first + j], w.corners)
        assert np.array_equal(s.map.collidable_centers[s.first + j], w.pos)
    # the static cone never moved, and the reset pose is valid with the walkers at home
    assert len(s.map.collidable_corners) == 4 and s.first == 1
    assert s._valid_pose(s.cur_pos, s.cur_angle, 1.3)
