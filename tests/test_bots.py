"""Lane-following bots on the CPU: the map loader behind `lane_bots=True`, its
tables, the table size, and the restatement the GPU tests compare against
(tests/bots_ref.py)."""
import math

import numpy as np
import pytest

import bots_ref as BR
import walkers_ref as WR
from oracle import dtsim_ref as R

ROWS = BR.FIXTURE_ROWS


def load(name, **kw):
    from aido1_amd.maps import load_map
    return load_map(name, **kw)


def custom(tmp_path, objects, **kw):
    return load(BR.write_map(tmp_path / 'm.yaml', objects), **kw)


@pytest.fixture(scope='module')
def path():
    """The restatement's own paths from home over the fixture's table."""
    return BR.own_path(BR.FIXTURE_TILES, BR.FIXTURE_OBJECTS, ROWS)


# ---- the loader ---------------------------------------------------------------------------
def test_bot_map_parses_with_the_switch(tmp_path):
    m = custom(tmp_path, BR.FIXTURE_OBJECTS, lane_bots=True)
    assert [(o.kind, o.static, o.bot, o.walker) for o in m.objects] == [
        ('duckiebot', False, True, False), ('cone', True, False, False),
        ('duckiebot', False, True, False), ('duckiebot', False, True, False)]
    assert not m.has_walkers and len(m.bots) == 3 and all(o.collidable for o in m.bots)
    assert [(o.velocity, o.follow_dist) for o in m.bots] == [(0.15, 0.3), (0.3, 0.25), (0.1, 0.3)]
    assert np.array_equal(m.bot_param_table[2], [0.1, 0.3, 2.0, 0.0, 0.0318, 27.0, 1.0])
    home = m.bot_home
    assert home.shape == (3, 3)
    assert np.array_equal(home[0], [0.61 * 1.5, 0.61 * 0.3, math.radians(180.0)])
    ref_bots = [BR.Bot(d, 0.61) for d in BR.split_objects(BR.FIXTURE_OBJECTS)[1]]
    assert np.array_equal(home, np.array([b.home for b in ref_bots]))


def test_without_the_switch_the_bot_is_refused(tmp_path):
    with pytest.raises(NotImplementedError, match='lane_bots'):
        custom(tmp_path, BR.FIXTURE_OBJECTS)
    with pytest.raises(NotImplementedError, match='lane_bots'):
        load('loop_dyn_duckiebots')
    # with it, any other dynamic kind is still refused
    with pytest.raises(NotImplementedError):
        custom(tmp_path, [dict(BR.BOT, kind='cone', pos=[1.5, 0.3])], lane_bots=True)
    for bad in (dict(velocity=-0.1), dict(follow_dist=0.0), dict(velocity=float('nan'))):
        with pytest.raises(ValueError):
            custom(tmp_path, [dict(BR.BOT, pos=[1.5, 0.3], **bad)], lane_bots=True)


def test_shipped_map_and_listing():
    from aido1_amd.maps import available_maps
    m = load('loop_dyn_duckiebots', lane_bots=True)
    assert 2 <= len(m.bots) <= 3 and len(m.objects) == len(m.bots)
    assert 'loop_dyn_duckiebots' not in available_maps()
    assert 'loop_dyn_duckiebots' in available_maps(lane_bots=True)
    assert set(available_maps()) < set(available_maps(lane_bots=True))
    # every bot starts on a lane centre, heading along it
    sim = R.SimulatorRef(m.rows)
    for x, z, a in m.bot_home:
        P, T = sim.closest_curve_point(np.array([x, 0.0, z]), a)
        assert np.hypot(P[0] - x, P[2] - z) < 2e-3
        assert R.get_dir_vec(a) @ T > 0.999


def test_table_order_statics_walkers_bots(tmp_path):
    objs = [dict(BR.BOT, pos=[1.5, 0.3], rotate=180),
            dict(WR.DUCKIE, pos=[1.5, 0.05], rotate=-90, static=False),
            dict(kind='cone', pos=[1.5, 2.5], height=0.1, mesh_min=[-0.35, 0.0, -0.35],
                 mesh_max=[0.35, 1.0, 0.35]),
            dict(BR.BOT, pos=[0.3, 1.5], rotate=-90)]
    m = custom(tmp_path, objs, lane_bots=True)
    ot = m.object_table
    assert ot.shape == (4, 20)
    order = [2, 1, 0, 3]      # the cone, the walker, then the bots in load order
    assert np.array_equal(ot[:, :3], np.array([m.objects[i].pos for i in order]))
    assert np.array_equal(m.bot_object_rows, [2, 3])
    assert np.array_equal(m.bot_render_rows, [0, 3])      # render_table keeps load order
    wt = m.walker_table
    assert wt[1, 4] >= 1 and not wt[[0, 2, 3]].any()      # the bots' walker rows are static
    assert m.has_walkers


def test_row_zero_is_the_static_record(tmp_path, path):
    m = custom(tmp_path, BR.FIXTURE_OBJECTS, lane_bots=True)
    twin = custom(tmp_path, BR.all_static(BR.FIXTURE_OBJECTS))
    rec = m.bot_records(path[:5])
    assert rec.shape == (5, 3, 20) and rec.dtype == np.float64
    for b, o in enumerate(m.bots):
        assert np.array_equal(rec[0, b], o.record())
    # ... which is dt_map.objects' row here, and the all-static twin's record
    # of the same object (the twin keeps load order: bot, cone, bot, bot)
    assert np.array_equal(m.object_table[m.bot_object_rows], rec[0])
    assert np.array_equal(m.object_table[0], twin.object_table[1])
    assert np.array_equal(rec[0], twin.object_table[[0, 2, 3]])
    ren = m.bot_render_records(path[:5])
    assert ren.shape == (5, 3, 8) and ren.dtype == np.float32
    assert np.array_equal(ren[0], m.render_table[m.bot_render_rows])
    assert np.array_equal(ren[0], twin.render_table[m.bot_render_rows])


def test_moving_rows_hold_the_agent_box(tmp_path, path):
    """Rows >= 1: agent_boundbox of the pose, generate_norm, _proj, the centre
    the pose -- against the oracle's own functions."""
    m = custom(tmp_path, BR.FIXTURE_OBJECTS, lane_bots=True)
    rows = [1, 2, 400, ROWS - 1]
    rec = m.bot_records(path)
    ren = m.bot_render_records(path)
    ref_bots = [BR.Bot(d, 0.61) for d in BR.split_objects(BR.FIXTURE_OBJECTS)[1]]
    for t in rows:
        for b, bot in enumerate(ref_bots):
            c, nm, centre = bot.box(t, path[t, b])
            r = rec[t, b]
            assert np.array_equal(r[0:3], centre) and r[3] == bot.safety_radius
            assert np.array_equal(r[4:12].reshape(4, 2), c)
            assert np.array_equal(r[12:16].reshape(2, 2), nm)
            for a in range(2):
                # (an ulp: numpy's matrix product rounds differently for the
                # oracle's strided axis and the record's contiguous one)
                p = c @ nm[a]
                assert abs(r[16 + 2 * a] - p.min()) <= 1e-15
                assert abs(r[17 + 2 * a] - p.max()) <= 1e-15
            e1, e2 = c[1] - c[0], c[3] - c[0]
            want = np.array([c[0, 0], c[0, 1], e1[0], e1[1], e2[0], e2[1], e1 @ e1, e2 @ e2])
            assert np.allclose(ren[t, b], want.astype(np.float32), rtol=1e-6, atol=0)
            assert np.array_equal(ren[t, b, :6], want[:6].astype(np.float32))
    # the box is the agent's: ROBOT_WIDTH x ROBOT_LENGTH
    c = rec[400, 0, 4:12].reshape(4, 2)
    assert abs(np.linalg.norm(c[1] - c[0]) - R.ROBOT_WIDTH) < 1e-12
    assert abs(np.linalg.norm(c[3] - c[0]) - R.ROBOT_LENGTH) < 1e-12


def test_agent_boundbox_is_the_oracles():
    from aido1_amd.maps import agent_boundbox
    rng = np.random.default_rng(0)
    for _ in range(20):
        p, a = rng.uniform(0, 2, 3), rng.uniform(-7, 7)
        f, r = R.get_dir_vec(a), R.get_right_vec(a)
        assert np.array_equal(agent_boundbox(p, 0.15, 0.18, f, r),
                              R.agent_boundbox(p, 0.15, 0.18, f, r))


# ---- the table's size ------------------------------------------------------------------
@pytest.mark.parametrize('cfg_kw', [dict(max_env_steps=7, repeat_actions=3),
                                    dict(max_env_steps=9, repeat_actions=2, frame_skip=2),
                                    dict(max_env_steps=50, repeat_actions=3, max_steps=20),
                                    dict(max_env_steps=5, repeat_actions=1, frame_skip=3,
                                         max_steps=17)])
def test_rows_cover_a_wrapped_run(cfg_kw):
    """EnvironmentWrapperRef on a tiny config, driven slowly along the lane so
    that episodes end by the counters: no env's step counter exceeds rows - 1,
    and the bound is reached."""
    from aido1_amd.maps import bot_rows
    cfg = R.SimConfig(**cfg_kw)
    rows = bot_rows(cfg.max_steps, cfg.frame_skip, cfg.max_env_steps)
    seen = 0
    for e in range(3):
        w = R.EnvironmentWrapperRef(R.SimulatorRef(BR.FIXTURE_TILES, 5, e, cfg))
        w.reset()
        for _ in range(60):
            _, _, done = w.step(np.array([0.01, 0.01], np.float32))
            seen = max(seen, w.sim.step_count)
            assert w.sim.step_count <= rows - 1
            if done:
                w.reset()
    assert seen == rows - 1


def test_default_config_rows():
    from aido1_amd.config import EnvConfig
    from aido1_amd.maps import MAX_BOT_ROWS, bot_rows
    c = EnvConfig()
    assert bot_rows(c.max_steps, c.frame_skip, c.max_env_steps) == 2002 <= MAX_BOT_ROWS


# ---- the restatement -------------------------------------------------------------------
def test_wheel_stage_is_the_oracles_wrapper():
    """bots_ref.wheels equals oracle.dtsim_ref.steering_to_wheels with the
    ActionWrapper's x0.8 on the left wheel undone."""
    rng = np.random.default_rng(1)
    for _ in range(200):
        vel, steer = rng.uniform(0, 0.5), rng.uniform(-6, 6)
        gain, trim, limit = rng.uniform(0.5, 3), rng.uniform(-0.2, 0.2), rng.uniform(0.2, 1.0)
        got = BR.wheels(vel, steer, R.WHEEL_DIST, gain=gain, trim=trim, limit=limit)
        ref = R.steering_to_wheels([vel, steer], gain=gain, trim=trim, limit=limit,
                                   wheel_dist=R.WHEEL_DIST)
        vels = np.array([ref[0] / 0.8, ref[1]])
        # (v * 0.8) / 0.8 is v or its neighbour; the right wheel is untouched
        assert got[1] == vels[1] and abs(got[0] - vels[0]) <= 2.3e-16 * abs(got[0])
    # the defaults are the bot's constants
    assert np.array_equal(BR.wheels(0.1, 0.0), np.full(2, 0.1 / 0.0318 * (2.0 / 27.0)))


def test_bots_stay_on_the_road_and_lap(path):
    sim = R.SimulatorRef(BR.FIXTURE_TILES)
    assert np.isfinite(path).all()
    for t in range(ROWS):
        for b in range(path.shape[1]):
            assert sim._drivable_pos(np.array([path[t, b, 0], 0.0, path[t, b, 1]])), (t, b)
    # at least one lap each: the heading turns through a full circle (the loop
    # is counter-clockwise: the angle grows), and the bot passes home again
    for b in range(path.shape[1]):
        assert path[-1, b, 2] - path[0, b, 2] >= 2 * math.pi, b
        d = np.hypot(path[200:, b, 0] - path[0, b, 0], path[200:, b, 1] - path[0, b, 1])
        assert d.min() < 0.02, (b, d.min())
    # and stays near the lane centre
    for t in range(0, ROWS, 50):
        for b in range(path.shape[1]):
            x, z, a = path[t, b]
            P, _ = sim.closest_curve_point(np.array([x, 0.0, z]), a)
            assert np.hypot(P[0] - x, P[2] - z) < 0.05, (t, b)


def test_undefined_paths_raise():
    sim = R.SimulatorRef(BR.FIXTURE_TILES)
    with pytest.raises(BR.PathUndefined):        # on the grass tile
        BR.bot_step(sim, 0.61 * 1.5, 0.61 * 1.5, 0.0, 0.1, 0.3)
    # heading off the map's edge from a straight: the follow point halves back
    # onto the road, so this one is defined
    BR.bot_step(sim, 0.61 * 1.5, 0.61 * 0.05, math.pi / 2, 0.1, 0.3)
