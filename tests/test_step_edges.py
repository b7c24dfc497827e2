"""The generated tile-edge and bisection-tie poses (tests/step_edges_ref.py):
that they reach what they are meant to reach, by the kernel's own predicates, so
that tests/test_gpu_step_edges.py cannot go quiet; and that on every one of them
the two CPU references, oracle/dtsim_ref.py and the C oracle, agree."""
import numpy as np
import pytest

import step_edges_ref as S
import walkers_ref as WR
from oracle import dtsim_ref as R
from oracle import oracle_c as OC

TOL = 1e-9      # the C oracle against dtsim_ref, as tests/test_oracle.py


@pytest.fixture(scope='module')
def cases():
    return S.cases()


def test_map_is_what_the_cases_need(cases, tmp_path):
    from aido1_amd import maps
    rows = S.tiles()
    assert len(rows) == S.H >= 11 and len(rows[0]) == S.W >= 11
    kinds = {t.split('/')[0] for row in rows for t in row}
    assert {'straight', 'curve_left', 'curve_right', '4way', '3way_left', 'grass'} <= kinds
    m = cases.map
    for q in range(S.BAD):      # 9 is not drivable next to a drivable 8, in x and in z
        assert m._get_tile(8, q)['drivable'] and not m._get_tile(S.BAD, q)['drivable']
        assert m._get_tile(q, 8)['drivable'] and not m._get_tile(q, S.BAD)['drivable']
    # the product loads both files; 128 B a curve, well inside dt_create's 48 KB of LDS
    for objects in ((), S.OBJECTS):
        tm = maps.load_map(S.write_map(tmp_path / 'edges.yaml', objects))
        assert (tm.width, tm.height) == (S.W, S.H)
        n_obj = len(tm.object_table)
        assert n_obj == len(objects) and tm.has_walkers == bool(objects)
        assert len(tm.curves) * 128 + 4096 < 48 * 1024 and S.W * S.H <= 256


def test_class_a_reaches_every_edge(cases):
    c = cases
    a = c.cls == 'A'
    for axis, edges in ((0, S.W), (1, S.H)):
        for k in range(edges + 1):
            for probe in range(5):
                sel = a & (c.axis == axis) & (c.k == k) & (c.probe == probe)
                assert (sel & c.in_window & ~c.control).any(), (axis, k, S.PROBES[probe])
                assert (sel & c.control).sum() >= 2
                assert set(c.angle[sel] == 0.0) == {True, False}
        # the one value where the reciprocal and the division give different tiles: a
        # probe on it keeps the pose valid where the reciprocal alone ends the episode,
        # and the pose on it is in column / row 8 where the reciprocal says 9
        d = a & (c.axis == axis) & c.differ
        assert d.any() and (c.k[d] == S.BAD).all() and c.in_window[d].all()
        assert (c.v[d] == S.step_ulps(S.BAD * S.TS, -1)).all()
        assert (d & c.div_valid & ~c.rcp_valid).any(), axis
        p = d & (c.probe == S.POSE)
        assert p.any() and (c.div_tile[p] != c.rcp_tile[p]).all() and (c.div_tile[p] >= 0).all()
    assert not (a & c.control & c.in_window).any()      # every +-2e-9 control is outside
    assert not (a & ~c.control & ~c.in_window).any()    # and everything else inside
    assert not c.rcp_valid[c.differ].any() and c.differ.sum() >= 10
    corner = c.cls == 'C'
    assert corner.sum() == 45 and c.in_window[corner].all() and c.differ[corner].any()


def test_class_b_reaches_every_level(cases):
    c = cases
    b = c.cls == 'B'
    for level in (1, 2, 3):     # the three `near` lines of bezier_closest_q's first round
        sel = b & (c.level == level)
        assert (sel & c.in_window).sum() >= 64, level
        assert (sel & c.flip).sum() >= 4, level
        assert (sel & c.control).any()
    assert not (c.flip & ~c.in_window).any()
    for level in range(4, 9):   # no floor: whatever the same scan finds
        sel = b & (c.level == level)
        print('level %d: %d in the window, %d flips' % (level, (sel & c.in_window).sum(),
                                                       (sel & c.flip).sum()))
    # recomputed from the pose alone, through the oracle's own bisection to that level
    for q in np.flatnonzero(b)[::7]:
        tile = c.map._get_tile(int(c.x[q] // S.TS), int(c.z[q] // S.TS))
        dots = R.tile_headings(tile['curves']) @ R.get_dir_vec(c.angle[q])
        cps = tile['curves'][int(np.argmax(dots))]
        pos = np.array([c.x[q], 0.0, c.z[q]])
        L = int(c.level[q])
        mid = R.bezier_closest(cps, pos, n=L - 1)
        h = 0.5 ** L
        pb, pt = R.bezier_point(cps, mid - h), R.bezier_point(cps, mid + h)
        db, dt = S.dist2(pb, c.x[q], c.z[q]), S.dist2(pt, c.x[q], c.z[q])
        assert bool(S.near_tie(db, dt)) == c.in_window[q]
        assert bool(S.flips(db, dt)) == c.flip[q]
        assert (R._norm3(pb - pos) < R._norm3(pt - pos)) == (np.sqrt(db) < np.sqrt(dt))


def test_class_t_walker_arrives_inside_the_decision(cases):
    c = cases
    t = np.flatnonzero(c.cls == 'T')
    assert len(t) == 16 and (c.step_count[t] >= 1).all()
    assert c.in_window[t].sum() == 12 and (c.control[t] == ~c.in_window[t]).all()
    sim = WR.WalkerSimRef(S.tiles(), objects=S.OBJECTS)
    for q in t:
        pos = np.array([c.x[q], 0.0, c.z[q]])
        ok = []
        for r in range(1, 4):
            sim.place(int(c.step_count[q]) + r)
            ok.append(sim._valid_pose(pos, c.angle[q]))
        first = int(c.r0[q])
        assert ok == [r < first for r in range(3)], (ok, first)
        sim.place(0)
        assert sim._valid_pose(pos, c.angle[q])     # a time of 0 would let it through


def test_class_u_bot_arrives_inside_the_decision(cases):
    c = cases
    u = np.flatnonzero(c.cls == 'U')
    assert len(u) == 16 and (c.step_count[u] >= 1).all()
    assert c.in_window[u].sum() == 12 and (c.control[u] == ~c.in_window[u]).all()
    sim, path = S.bot_sim()
    assert np.ptp(path[:, 0, 1]) > 0.2      # the bot drives
    for q in u:
        for dz in (-1e-6, 0.0, 1e-6):       # not on the brink: the device's own path will do
            pos = np.array([c.x[q], 0.0, c.z[q] + dz])
            ok = []
            for r in range(1, 4):
                sim.place(int(c.step_count[q]) + r)
                ok.append(sim._valid_pose(pos, c.angle[q]))
            assert ok == [r < int(c.r0[q]) for r in range(3)], (ok, c.r0[q], dz)
        sim.place(0)
        assert sim._valid_pose(pos, c.angle[q])


def test_waves_mix_flagged_and_plain(cases):
    c = cases
    assert c.n % 16 == 0 and 3000 <= c.n <= 6000
    groups = c.near.reshape(-1, 16)
    mixed = groups.any(1) & ~groups.all(1)
    assert mixed.mean() >= 0.9      # 16 envs = one wave of the fan kernel
    assert 0.2 <= (~c.near).mean() <= 0.8
    sub = cases.subset(c.cls == 'T')
    assert len(sub) == 16 and (c.cls[sub] == 'T').all()


def _python_step(sim, c, q):
    pos = np.array([c.x[q], 0.0, c.z[q]])
    sim.cur_pos, sim.cur_angle = pos.copy(), float(c.angle[q])
    sim.step_count, sim.speed = int(c.step_count[q]), 0.0
    w = R.EnvironmentWrapperRef(sim)
    valid = sim._valid_pose(pos, sim.cur_angle)
    lp0 = w.lane_pos()
    reward, reward_mod, done = w.step([0.0, 0.0])
    assert np.array_equal(sim.cur_pos, pos) and sim.cur_angle == c.angle[q]   # it stood still
    return valid, lp0, reward, reward_mod, done, w.lane_pos(), w.tile_index()


def _same_lane_pos(lp, row):
    if lp is None:
        return bool(np.isnan(row).all())
    return bool(np.max(np.abs(np.array(lp) - row) / np.array([1, 1, 57.3, 1])) <= TOL)


@pytest.mark.parametrize('objects', [False, True], ids=['empty', 'cone'])
def test_the_two_references_agree(cases, objects):
    """_valid_pose, get_lane_pos2 and one wrapper step at zero wheel velocities,
    dtsim_ref.py against the C oracle: done and tile exactly, rewards and the
    lane pose to 1e-9.  Every pose on the object-free map; every fourth one
    (and class T) beside the cone."""
    c = cases
    objs = [S.CONE] if objects else []
    idx = np.arange(c.n) if not objects else c.subset((np.arange(c.n) % 4 == 0) | (c.cls == 'T'))
    n = len(idx)
    ob = OC.OracleBatch(S.tiles(), n, auto_reset=False, objects=objs)
    ob.set_state(x=c.x[idx], z=c.z[idx], angle=c.angle[idx], step_count=c.step_count[idx])
    lp0, tile0 = ob.lane_pos()
    ref = ob.step(np.zeros((n, 2), np.float32))
    sim = R.SimulatorRef(S.tiles(), objects=objs)
    for e, q in enumerate(idx):
        valid, plp0, reward, reward_mod, done, plp, tile = _python_step(sim, c, q)
        assert valid == (not ref['done'][e]) and done == bool(ref['done'][e]), q
        assert tile == ref['tile'][e] == tile0[e], q
        assert abs(reward - ref['reward'][e]) <= TOL and \
            abs(reward_mod - ref['reward_mod'][e]) <= TOL, q
        assert _same_lane_pos(plp0, lp0[e]) and _same_lane_pos(plp, ref['lanepos'][e]), q
    # where the two floors differ both references take the division's answer
    d = np.flatnonzero(c.differ[idx])
    assert len(d) and np.array_equal(ref['done'][d] == 0, c.div_valid[idx][d])
    assert np.array_equal(ref['tile'][d], c.div_tile[idx][d])
