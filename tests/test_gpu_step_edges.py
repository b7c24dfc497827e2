"""GPU: the step kernels' rare exact paths (csrc/dtsim_common.h: floor_div_exact
behind floor_div_ts / floor_div_fast, root_less_exact behind root_less and the
`near` lines of bezier_closest_fast / bezier_closest_q, and the fallbacks of
valid_pose_q, lane_pos_q, lane_pos_lean) on the poses of tests/step_edges_ref.py:
probe points on tile edges and bisection ties, which random trajectories never
reach.  tests/test_step_edges.py shows on the CPU that the poses are inside the
windows and that the references agree on them.

The poses are set into the env and the oracle and the action is zero wheel
velocities, so every Simulator step of a decision (and each of the fan
kernel's three poses) tests the injected pose.  Each launch form against the
oracle as tests/test_gpu_step.py does: done, tile, counters and respawns
exactly, rewards and the lane pose within its TOL_TIGHT.

Left out: the spawn path (spawn_try's proposals cannot be injected;
test_reset_bit_exact stays its coverage).
"""
import numpy as np
import pytest
import torch

import bots_ref as BR
import step_edges_ref as S
import walkers_ref as WR
from oracle import dtsim_ref as R
from oracle import oracle_c as OC
from test_gpu_step import TOL_SPEC, TOL_TIGHT, compare_out, compare_state

pytestmark = pytest.mark.gpu

SEED = 1234


@pytest.fixture(scope='module')
def cases():
    return S.cases()


@pytest.fixture(scope='module')
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp('edges')
    return {'empty': S.write_map(d / 'edges.yaml'),
            'cone': S.write_map(d / 'edges_cone.yaml', [S.CONE]),
            'walker': S.write_map(d / 'edges_walker.yaml', S.OBJECTS),
            'bot': S.write_map(d / 'edges_bot.yaml', S.BOT_OBJECTS)}


def make_pair(path, n, objects=(), **cfg_kw):
    """test_gpu_step.make_pair for a map file of the test's own."""
    from aido1_amd.config import EnvConfig
    from aido1_amd.vec_env import VecEnv
    ec = EnvConfig(map_name=path, **cfg_kw)
    env = VecEnv(n, seed=SEED, config=ec)
    sc = R.SimConfig(**{k: v for k, v in cfg_kw.items() if k in R.SimConfig().__dict__})
    assert not sc.reward_speed_measured      # the nominal speed: dot_dir reaches the reward
    ob = OC.OracleBatch(S.tiles(), n, seed=SEED, sim_config=sc, auto_reset=ec.auto_reset,
                        objects=list(objects))
    return env, ob


def inject(env, ob, c, idx):
    env.reset()
    ob.reset()
    compare_state(env, ob, 0.0)
    s = dict(x=c.x[idx], z=c.z[idx], angle=c.angle[idx], step_count=c.step_count[idx])
    ob.set_state(**s)
    env.set_state(**s)


def who(c, idx, bad):
    """The envs of a mismatch by what they are, for the assertion's message."""
    q = idx[np.flatnonzero(bad)]
    tags = [('edge, floors differ', np.isin(c.cls[q], ('A', 'C', 'T', 'U')) & c.differ[q]),
            ('edge, in the window', np.isin(c.cls[q], ('A', 'C', 'T', 'U')) & ~c.differ[q] &
             c.in_window[q]),
            ('tie, flip', c.flip[q]), ('tie, in the window', c.in_window[q] & ~c.flip[q] &
                                       (c.cls[q] == 'B')),
            ('control or plain', c.control[q])]
    return '%d envs: ' % len(q) + ', '.join('%s %d' % (t, m.sum()) for t, m in tags if m.any())


def same(got, want, c, idx, what):
    bad = got != want
    assert not bad.any(), '%s: %s' % (what, who(c, idx, bad))


def close(got, want, c, idx, what, tol=TOL_TIGHT):
    bad = ~(np.abs(got - want) <= tol)
    assert not bad.any(), '%s: max err %g; %s' % (what, np.max(np.abs(got - want)),
                                                  who(c, idx, bad))


def check_oracle(c, idx, ref, ob):
    """On the oracle's own output, so that no case degenerates: an env that did
    not finish stands where it was put, and where the two floors differ done
    and tile are the division's answer, not the reciprocal's."""
    st = ob.state()
    keep = ref['done'] == 0
    for k in ('x', 'z', 'angle'):
        assert np.array_equal(st[k][keep], getattr(c, k)[idx][keep]), k
    assert 0.1 < keep.mean() < 0.9
    d = np.flatnonzero(c.differ[idx])
    q = idx[d]
    assert np.array_equal(ref['done'][d] == 0, c.div_valid[q])
    assert np.array_equal(ref['tile'][d], c.div_tile[q])
    assert (c.div_valid[q] != c.rcp_valid[q]).any() and (c.div_tile[q] != c.rcp_tile[q]).any()


def test_dt_step_and_lane_pos(gpu, cases, paths):
    """dt_lane_pos right after set_state (lane_pos_lean), then dt_step
    (step_kernel: floor_div_ts and root_less, the exact-form instantiation)."""
    c = cases
    idx = np.arange(c.n)
    env, ob = make_pair(paths['empty'], c.n)
    inject(env, ob, c, idx)
    lp, tile = env.lane_pos()
    rlp, rtile = ob.lane_pos()
    torch.cuda.synchronize()
    lp = lp.cpu().numpy()
    same(tile.cpu().numpy(), rtile, c, idx, 'dt_lane_pos tile')
    same(np.isnan(lp[:, 0]), np.isnan(rlp[:, 0]), c, idx, 'dt_lane_pos in lane')
    m = ~np.isnan(lp)
    assert m.any() and (~m).any() and np.array_equal(m, ~np.isnan(rlp))
    close(np.nan_to_num(lp[:, 0]), np.nan_to_num(rlp[:, 0]), c, idx, 'dt_lane_pos dist')
    close(np.nan_to_num(lp[:, 1]), np.nan_to_num(rlp[:, 1]), c, idx, 'dt_lane_pos dot_dir')
    assert np.max(np.abs(lp[m] - rlp[m])) <= TOL_TIGHT * 1e3     # compare_out's bound
    zero = np.zeros((c.n, 2), np.float32)
    out = env.step_into(torch.from_numpy(zero).to(gpu))
    ref = ob.step(zero)
    torch.cuda.synchronize()
    check_oracle(c, idx, ref, ob)
    same(out.done.cpu().numpy(), ref['done'], c, idx, 'dt_step done')
    same(out.tile.cpu().numpy(), ref['tile'], c, idx, 'dt_step tile')
    close(out.reward.cpu().numpy(), ref['reward'], c, idx, 'dt_step reward')
    assert compare_out(out, ref) <= TOL_SPEC
    compare_state(env, ob)
    env.check()


def run_many(gpu, env, ob, c, idx, k, check_first=True):
    from aido1_amd.vec_env import StepOutput
    n = len(idx)
    out = StepOutput(k * n, gpu, lanepos=False, tile=False)
    zero = np.zeros((k, n, 2), np.float32)
    env.step_many_into(torch.from_numpy(zero).to(gpu), out)
    torch.cuda.synchronize()
    rew, rewm, done = (t.view(k, n).cpu().numpy() for t in (out.reward, out.reward_mod, out.done))
    obs = out.obs.view(k, n, 2).cpu().numpy()
    for d in range(k):
        # the later decisions run on what the first left, respawns included
        ref = ob.step(zero[d])
        if d == 0 and check_first:
            check_oracle(c, idx, ref, ob)
        same(done[d], ref['done'], c, idx, 'dt_step_many done, decision %d' % d)
        close(rew[d], ref['reward'], c, idx, 'dt_step_many reward, decision %d' % d)
        close(rewm[d], ref['reward_mod'], c, idx, 'dt_step_many reward_mod, decision %d' % d)
        assert np.max(np.abs(obs[d] - ref['obs'])) <= 1e-6, d
    compare_state(env, ob)
    env.check()


@pytest.mark.parametrize('k', [1, 3])
def test_step_many_fan_lean(gpu, cases, paths, k):
    """dt_step_many on the object-free map: step_fan_kernel<true> (valid_pose_q,
    lane_pos_q, bezier_closest_q); the shuffled batch puts flagged and plain
    quads into the same waves."""
    c = cases
    idx = np.arange(c.n)
    env, ob = make_pair(paths['empty'], c.n)
    inject(env, ob, c, idx)
    run_many(gpu, env, ob, c, idx, k)


def test_step_many_fan_objects(gpu, cases, paths):
    """The same beside a collidable object: step_fan_kernel<false>."""
    c = cases
    idx = np.arange(c.n)
    env, ob = make_pair(paths['cone'], c.n, [S.CONE])
    assert len(env.map.object_table) == 1 and not env.map.has_walkers
    inject(env, ob, c, idx)
    run_many(gpu, env, ob, c, idx, 2)


def test_step_many_generic_route(gpu, cases, paths):
    """repeat_actions = 4, more Simulator steps than the fan kernel holds:
    dt_step_many runs step_kernel over the decisions."""
    c = cases
    idx = np.arange(c.n)
    env, ob = make_pair(paths['empty'], c.n, repeat_actions=4)
    inject(env, ob, c, idx)
    run_many(gpu, env, ob, c, idx, 2)


@pytest.mark.parametrize('mover', ['walker', 'bot'])
def test_mover_time_reaches_the_fallback(gpu, cases, paths, mover):
    """A walker (a lane-following bot) on the map and step counters injected:
    the kWalk (kBot) instantiations of step_kernel (dt_step) and
    step_fan_kernel (dt_step_many) against tests/walkers_ref.py
    (tests/bots_ref.py).  Class T (U) stands on a tile edge in the mover's way,
    so valid_pose_q's fallback runs valid_pose<kWalk, kBot>(..., t) and t must
    be step_count + r: the mover arrives at step 1, 2, 3 or not at all.  The
    rest of the batch (the reference is Python, an env at a time): every pose
    where the two floors differ, every third flip of levels 1 to 3, every 48th
    of the others, each at a step counter of its own (a bot's beyond its table
    too, where it stands on the last row)."""
    from aido1_amd.vec_env import StepOutput, VecEnv
    from aido1_amd.config import EnvConfig
    c = cases
    cls = 'T' if mover == 'walker' else 'U'
    flip = np.flatnonzero(c.flip & (c.level <= 3))[::3]
    idx = c.subset((c.cls == cls) | c.differ | np.isin(np.arange(c.n), flip) |
                   (np.arange(c.n) % 48 == 0))
    n = len(idx)
    assert n <= 256 and len(flip) >= 64
    t0 = c.step_count[idx].copy()
    other = c.cls[idx] != cls
    t0[other] = (1 + 7 * np.arange(n) % 50)[other]
    if mover == 'walker':
        ref = WR.WalkerBatchRef(S.tiles(), S.OBJECTS, n, SEED)
        kw = {}
    else:
        path = S.bot_sim()[1]
        ref = BR.BotBatchRef(S.tiles(), S.BOT_OBJECTS, path, n, SEED)
        kw = dict(lane_bots=True, bot_rows=S.BOT_ROWS)
    ref.reset()
    for w, x, z, a in zip(ref.envs, c.x[idx], c.z[idx], c.angle[idx]):
        w.sim.cur_pos, w.sim.cur_angle = np.array([x, 0.0, z]), float(a)
    ref.set_step_count(t0)
    zero = np.zeros((n, 2), np.float32)
    want = ref.step(zero)
    end = ref.state()
    # the class on the reference: the mover ends the decision at step r0 + 1, in the
    # window and out of it alike, and each arrival is a reward of its own
    t = np.flatnonzero(c.cls[idx] == cls)
    assert len(t) == 16 and np.array_equal(want['done'][t], c.r0[idx][t] < 3)
    by_r0 = [want['reward'][t][c.r0[idx][t] == r] for r in range(4)]
    assert all(np.ptp(v) <= 1e-6 for v in by_r0)     # (x differs by up to 2e-9 among them)
    assert len({round(float(v[0]), 6) for v in by_r0}) == 4
    assert (ref.walker_ends if mover == 'walker' else ref.bot_ends) >= 12
    d = np.flatnonzero(c.differ[idx])
    assert np.array_equal(want['done'][d] == 0, c.div_valid[idx][d])
    for many in (False, True):
        env = VecEnv(n, seed=SEED, config=EnvConfig(map_name=paths[mover]), **kw)
        if mover == 'walker':
            assert env.map.has_walkers
        else:
            assert np.max(np.abs(env.bot_path - path)) <= TOL_TIGHT
        env.reset()
        env.set_state(x=c.x[idx], z=c.z[idx], angle=c.angle[idx], step_count=t0)
        if many:
            out = StepOutput(n, gpu, lanepos=False, tile=False)
            env.step_many_into(torch.from_numpy(zero[None]).to(gpu), out)
        else:
            out = env.step_into(torch.from_numpy(zero).to(gpu))
        torch.cuda.synchronize()
        form = 'dt_step_many' if many else 'dt_step'
        same(out.done.cpu().numpy(), want['done'], c, idx, form + ' done')
        if not many:
            same(out.tile.cpu().numpy(), want['tile'], c, idx, form + ' tile')
        close(out.reward.cpu().numpy(), want['reward'], c, idx, form + ' reward')
        close(out.reward_mod.cpu().numpy(), want['reward_mod'], c, idx, form + ' reward_mod')
        g = env.get_state()
        for k in ('x', 'z', 'angle'):
            assert np.max(np.abs(g[k] - end[k])) <= TOL_TIGHT, (many, k)
        assert np.array_equal(g['step_count'], end['step_count']), many
        env.check()
