"""GPU: lane-following bots (dt_bot_path / dt_set_bots / dt_render_bots) -- the
path kernel a step at a time against the CPU restatement of tests/bots_ref.py,
then both step kernels and the render's object phase with the restatement fed
the device's own path (steps: done and tile exact, rewards within 1e-9, the
project's bound for GPU against oracle, tests/test_gpu_step.py; frames: bit for
bit against tests/render_objects_ref.py's composition).

The fixture (bots_ref.FIXTURE_*) was chosen on the CPU, on the restatement's
own path: of 496 episode ends in the 96 x 40 run below 94 are bot hits away
from home, and 609 of 3840 decisions carry a negative proximity penalty."""
import ctypes

import numpy as np
import pytest
import torch

import bots_ref as BR
import render_objects_ref as RO
import walkers_ref as WR
from oracle import dtsim_ref as R
from oracle import oracle_c as OC

pytestmark = pytest.mark.gpu

TOL = 1e-9
SEED = 2024
N, DEC, K_MANY = 96, 40, 8     # six fan workgroups / a partial step_kernel block
ROWS = BR.FIXTURE_ROWS
F = np.float32
vp = ctypes.c_void_p

# the all-static twin in dt_map.objects' order (statics, then the bots), so that
# the penalty sums over the same rows in the same order
TWIN = [o for o in BR.all_static(BR.FIXTURE_OBJECTS) if o['kind'] != 'duckiebot'] + \
    [o for o in BR.all_static(BR.FIXTURE_OBJECTS) if o['kind'] == 'duckiebot']


@pytest.fixture(scope='module')
def map_path(tmp_path_factory):
    return BR.write_map(tmp_path_factory.mktemp('bots') / 'bots.yaml')


@pytest.fixture(scope='module')
def static_path(tmp_path_factory):
    return BR.write_map(tmp_path_factory.mktemp('bots') / 'static_twin.yaml', TWIN)


def make_env(path, n, seed=SEED, draw=False, lane_bots=True, bot_rows=ROWS, **cfg_kw):
    from aido1_amd.config import EnvConfig
    from aido1_amd.vec_env import VecEnv
    return VecEnv(n, seed=seed, config=EnvConfig(map_name=path, **cfg_kw), draw_objects=draw,
                  lane_bots=lane_bots, bot_rows=bot_rows)


def ptr(a):
    return a.ctypes.data_as(vp)


def _err(env):
    return env._L.dt_last_error(env._h).decode()


@pytest.fixture(scope='module')
def dev_path(gpu, map_path):
    """The device's paths [ROWS, 3, 3]: what every later test feeds the restatement."""
    env = make_env(map_path, 8)
    path = env.bot_path.copy()
    env.close()
    assert path.shape == (ROWS, 3, 3) and np.isfinite(path).all()
    return path


# ---- the path ---------------------------------------------------------------------------
def test_path_one_step_at_a_time(dev_path):
    """From the device's row t the restatement's single step gives the device's
    row t + 1 within 1e-9 -- no accumulation, so the project's own bound."""
    sim = R.SimulatorRef(BR.FIXTURE_TILES)
    bots = [BR.Bot(d, 0.61) for d in BR.split_objects(BR.FIXTURE_OBJECTS)[1]]
    assert np.array_equal(dev_path[0], np.array([b.home for b in bots]))
    worst = 0.0
    for b, bot in enumerate(bots):
        for t in range(ROWS - 1):
            want = BR.bot_step(sim, *dev_path[t, b], bot.velocity, bot.follow_dist)
            worst = max(worst, float(np.max(np.abs(np.array(want) - dev_path[t + 1, b]))))
    print('bot path, one step from the device\'s row: max |diff| %.3g' % worst)
    assert worst <= TOL


def test_path_end_to_end_is_reported(dev_path):
    """The device's whole path against the restatement's own from home, 1000
    steps of a closed loop: recorded, not gated (nothing else depends on it)."""
    own = BR.own_path(BR.FIXTURE_TILES, BR.FIXTURE_OBJECTS, ROWS)
    d = np.abs(own - dev_path)
    print('bot path, end to end over %d rows: max |diff| %.3g (x, z %.3g; angle %.3g)'
          % (ROWS, d.max(), d[..., :2].max(), d[..., 2].max()))
    assert np.isfinite(d).all()


# ---- steps ------------------------------------------------------------------------------
class Run:
    """The restatement's run on the device's path: n envs reset, every
    step_count set to U{lo..hi-1} (the first ones to `first`), `dec`
    decisions of actions U[0.3, 1)^2.  Computed once, never changed."""

    def __init__(self, path, n, dec, rng_seed, lo=0, hi=1000, rows=ROWS, first=(),
                 objects=BR.FIXTURE_OBJECTS, **cfg_kw):
        rng = np.random.default_rng(rng_seed)
        self.n, self.dec, self.rows, self.cfg_kw = n, dec, rows, cfg_kw
        self.ref = BR.BotBatchRef(BR.FIXTURE_TILES, objects, path[:rows], n, SEED, **cfg_kw)
        self.ref.reset()
        self.start = self.ref.state()
        self.t0 = rng.integers(lo, hi, n).astype(np.uint32)
        self.t0[:len(first)] = first
        self.ref.set_step_count(self.t0)
        self.actions = rng.uniform(0.3, 1.0, (dec, n, 2)).astype(F)
        self.outs = [self.ref.step(self.actions[d]) for d in range(dec)]
        self.end = self.ref.state()

    def fresh_env(self, path, **kw):
        env = make_env(path, self.n, bot_rows=self.rows, **self.cfg_kw, **kw)
        env.reset()
        g = env.get_state()
        for k in ('x', 'z', 'angle'):
            assert np.array_equal(g[k], self.start[k]), k
        env.set_state(step_count=self.t0)
        return env

    def check(self, d, reward, reward_mod, done, tile=None):
        want = self.outs[d]
        assert np.array_equal(done, want['done']), d
        if tile is not None:
            assert np.array_equal(tile, want['tile']), d
        er = np.max(np.abs(reward - want['reward']))
        em = np.max(np.abs(reward_mod - want['reward_mod']))
        assert er <= TOL and em <= TOL, (d, er, em)

    def check_end(self, env):
        g = env.get_state()
        for k in ('x', 'z', 'angle'):
            assert np.max(np.abs(g[k] - self.end[k])) <= TOL, k
        assert np.array_equal(g['step_count'], self.end['step_count'])
        env.check()

    def drive(self, env, gpu, many):
        from aido1_amd.vec_env import StepOutput
        if not many:
            for d in range(self.dec):
                out = env.step_into(torch.from_numpy(self.actions[d]).to(gpu))
                torch.cuda.synchronize()
                self.check(d, out.reward.cpu().numpy(), out.reward_mod.cpu().numpy(),
                           out.done.cpu().numpy(), out.tile.cpu().numpy())
        else:
            out = StepOutput(K_MANY * self.n, gpu, lanepos=False, tile=False)
            for d0 in range(0, self.dec, K_MANY):
                a = torch.from_numpy(np.ascontiguousarray(self.actions[d0:d0 + K_MANY])).to(gpu)
                env.step_many_into(a, out)
                torch.cuda.synchronize()
                r, rm, dn = (t.cpu().numpy().reshape(K_MANY, self.n)
                             for t in (out.reward, out.reward_mod, out.done))
                for i in range(K_MANY):
                    self.check(d0 + i, r[i], rm[i], dn[i])
        self.check_end(env)


@pytest.fixture(scope='module')
def run(dev_path):
    r = Run(dev_path, N, DEC, 7)
    # not vacuous, on the restatement's own results: bots away from home end
    # episodes, and the penalty is at work
    ref = r.ref
    print('episode ends %d, of them bot hits away from home %d; decisions %d, negative '
          'penalty %d' % (ref.ends, ref.bot_ends, ref.decisions, ref.negative))
    assert ref.bot_ends >= 0.05 * ref.ends > 0
    assert ref.negative >= 0.05 * ref.decisions
    return r


def test_step_parity_step_kernel(gpu, run, map_path):
    """dt_step: step_kernel's bot instantiation, a partial block."""
    run.drive(run.fresh_env(map_path), gpu, many=False)


def test_step_parity_fan_kernel(gpu, run, map_path):
    """dt_step_many at k = 8: step_fan_kernel's bot instantiation, wave 0
    testing the decision's three poses at t + 1, t + 2, t + 3."""
    run.drive(run.fresh_env(map_path), gpu, many=True)


@pytest.fixture(scope='module')
def clamp_run(dev_path):
    r = Run(dev_path, 64, 16, 11, lo=50, hi=400, rows=50, first=np.arange(42, 50))
    assert r.ref.ends > 0 and r.ref.negative > 0
    return r


@pytest.mark.parametrize('many', [False, True], ids=['step_kernel', 'fan_kernel'])
def test_clamp_past_the_table(gpu, clamp_run, dev_path, map_path, many):
    """A 50-row table with step counts past it (and eight inside, crossing its
    end): the restatement freezes the bots at row 49."""
    r = clamp_run
    env = r.fresh_env(map_path)
    assert env.bot_path.shape == (50, 3, 3) and np.array_equal(env.bot_path, dev_path[:50])
    r.drive(env, gpu, many)


def test_table_of_home_rows_equals_the_static_twin(gpu, dev_path, map_path, static_path):
    """dt_set_bots with every row the bots' row 0: rewards, done and state
    equal, bit for bit, the same map with the entries `static: true` and no
    bots (the kernels without movers)."""
    from aido1_amd.vec_env import StepOutput
    n, dec = 64, 12
    rng = np.random.default_rng(4)
    acts = torch.from_numpy(rng.uniform(0.3, 1.0, (dec, n, 2)).astype(F)).to(gpu)
    t0 = rng.integers(0, 300, n).astype(np.uint32)
    results = []
    for bots in (False, True):
        env = make_env(map_path if bots else static_path, n, lane_bots=bots, bot_rows=64)
        assert len(env.map.bots) == (3 if bots else 0) and len(env.map.object_table) == 4
        if bots:
            rec = env.map.bot_records(np.repeat(dev_path[:1], 64, 0))
            rec[:] = rec[0]
            row = np.ascontiguousarray(env.map.bot_object_rows, np.int32)
            assert env._L.dt_set_bots(env._h, ptr(rec), ptr(row), 64, 3) == 0, _err(env)
        env.reset()
        env.set_state(step_count=t0)
        res = []
        for d in range(4):
            o = env.step_into(acts[d])
            res += [o.reward.clone(), o.reward_mod.clone(), o.done.clone(), o.tile.clone()]
        many = StepOutput((dec - 4) * n, gpu, lanepos=False, tile=False)
        env.step_many_into(acts[4:].contiguous(), many)
        res += [many.reward, many.reward_mod, many.done]
        torch.cuda.synchronize()
        env.check()
        st = env.get_state()
        res += [torch.from_numpy(st[k]) for k in sorted(st)]
        results.append(res)
    for i, (a, b) in enumerate(zip(*results)):
        assert torch.equal(a, b), i
    assert any(bool(r.any()) for r in results[0][2:16:4])    # some episode ended
    assert bool((results[0][16] != 0).any())


# ---- walkers and bots on one map --------------------------------------------------------
MROWS = 400


@pytest.fixture(scope='module')
def mixed_path(tmp_path_factory):
    return BR.write_map(tmp_path_factory.mktemp('bots') / 'mixed.yaml', BR.MIXED_OBJECTS)


@pytest.fixture(scope='module')
def mixed_dev_path(gpu, mixed_path):
    env = make_env(mixed_path, 8, bot_rows=MROWS)
    assert env.map.has_walkers and list(env.map.bot_object_rows) == [2, 3]
    path = env.bot_path.copy()
    env.close()
    return path


@pytest.fixture(scope='module')
def mixed_run(mixed_dev_path):
    r = Run(mixed_dev_path, 48, 16, 13, hi=MROWS, rows=MROWS, objects=BR.MIXED_OBJECTS)
    assert r.ref.ends > 0 and r.ref.bot_ends > 0 and r.ref.negative > 0
    return r


@pytest.mark.parametrize('many', [False, True], ids=['step_kernel', 'fan_kernel'])
def test_step_parity_with_a_walker_and_bots(gpu, mixed_run, mixed_path, many):
    """The bot instantiations stage the walker rows too: a walker row moves by
    its closed form, a bot row comes from the table, in one launch."""
    mixed_run.drive(mixed_run.fresh_env(mixed_path), gpu, many)


# ---- graph, reset, state ----------------------------------------------------------------
def test_graph_outlives_switching_the_bots_off(gpu, run, dev_path, map_path, static_path):
    """A graph captured with bots on, replayed, the bots switched off
    (dt_set_bots n = 0 frees the table), replayed again: the second replay
    sees every object static -- bit for bit the all-static twin from the same
    state -- and reads nothing of the freed table."""
    from aido1_amd.vec_env import StepOutput
    acts = torch.from_numpy(np.ascontiguousarray(run.actions[:12])).to(gpu)
    env = run.fresh_env(map_path)
    buf = acts[:6].clone()
    out = StepOutput(N, gpu)
    graph = env.capture(buf, out)
    graph.replay()
    torch.cuda.synchronize()
    run.check(5, out.reward.cpu().numpy(), out.reward_mod.cpu().numpy(), out.done.cpu().numpy())
    st = env.get_state()
    assert env._L.dt_set_bots(env._h, None, None, 0, 0) == 0, _err(env)
    # fresh allocations of the freed table's size: stale reads would not see zeros
    junk = [torch.full((ROWS * 3 * 20,), 1e30, dtype=torch.float64, device=gpu) for _ in range(3)]
    twin = make_env(static_path, N, lane_bots=False)
    twin.reset()
    twin.set_state(**st)
    buf.copy_(acts[6:12])
    graph.replay()
    torch.cuda.synchronize()
    for d in range(6, 12):
        o = twin.step_into(acts[d])
    torch.cuda.synchronize()
    assert torch.equal(out.reward, o.reward) and torch.equal(out.reward_mod, o.reward_mod)
    assert torch.equal(out.done, o.done) and torch.equal(out.tile, o.tile)
    a, b = env.get_state(), twin.get_state()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # ... and differs from the run with the bots on
    assert np.max(np.abs(out.reward.cpu().numpy() - run.outs[11]['reward'])) > 1e-6
    del junk
    env.check()
    twin.check()


def test_graph_replay_equals_eager(gpu, run, map_path):
    """A captured graph of 6 dt_step launches replayed twice equals 12 eager
    steps: nothing about the bots is decided on the host per launch."""
    from aido1_amd.vec_env import StepOutput
    acts = torch.from_numpy(np.ascontiguousarray(run.actions[:12])).to(gpu)
    eager = run.fresh_env(map_path)
    outs = []
    for d in range(12):
        o = eager.step_into(acts[d])
        torch.cuda.synchronize()
        outs.append((o.reward.clone(), o.reward_mod.clone(), o.done.clone()))
        run.check(d, o.reward.cpu().numpy(), o.reward_mod.cpu().numpy(), o.done.cpu().numpy())
    env = run.fresh_env(map_path)
    buf = acts[:6].clone()
    out = StepOutput(N, gpu)
    graph = env.capture(buf, out)
    for rep in range(2):
        buf.copy_(acts[6 * rep:6 * rep + 6])
        graph.replay()
        torch.cuda.synchronize()
        last = outs[6 * rep + 5]
        assert torch.equal(out.reward, last[0]) and torch.equal(out.reward_mod, last[1])
        assert torch.equal(out.done, last[2])
    a, b = eager.get_state(), env.get_state()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    env.check()


def test_state_round_trip_carries_the_bots(gpu, run, map_path):
    """get_state after 5 decisions, set_state into a fresh handle: both go on
    to the same results (the bots' poses come with step_count)."""
    acts = torch.from_numpy(np.ascontiguousarray(run.actions[:10])).to(gpu)
    a = run.fresh_env(map_path)
    for d in range(5):
        a.step_into(acts[d])
    torch.cuda.synchronize()
    st = a.get_state()
    b = make_env(map_path, N)
    b.reset()
    b.set_state(**st)     # (with the episode counters: the spawn-ahead follows them)
    for d in range(5, 10):
        oa, ob = a.step_into(acts[d]), b.step_into(acts[d])
        torch.cuda.synchronize()
        assert torch.equal(oa.reward, ob.reward) and torch.equal(oa.done, ob.done), d
        assert torch.equal(oa.reward_mod, ob.reward_mod) and torch.equal(oa.tile, ob.tile), d
        run.check(d, ob.reward.cpu().numpy(), ob.reward_mod.cpu().numpy(),
                  ob.done.cpu().numpy(), ob.tile.cpu().numpy())
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    a.check()
    b.check()


# ---- frames -----------------------------------------------------------------------------
NF = 64


class Scene:
    """64 poses around the bots where their env's step count puts them (some
    counts past the table: clamped), and the expected frames: the oracle's
    object-free frame, each env's records painted red, the oracle's line
    detector on that image."""

    def __init__(self, path, dev_path):
        from aido1_amd.maps import load_map
        m = load_map(path, lane_bots=True)
        self.table = m.render_table
        self.rows = m.bot_render_rows
        self.recs = m.bot_render_records(dev_path)
        assert self.recs.dtype == F and self.recs.shape == (ROWS, 3, 8)
        rng = np.random.default_rng(21)
        self.t = rng.integers(0, ROWS, NF).astype(np.uint32)
        self.t[1] = (self.t[0] + 300) % ROWS     # env 1: env 0's pose at another time
        self.t[2:6] = [ROWS - 1, ROWS, ROWS + 7, 500000]     # the clamp
        centres = []
        for i in range(NF):
            tt = min(int(self.t[i]), ROWS - 1)
            centres.append(tuple(dev_path[tt, i % 3, :2]))
        self.x, self.z, self.a = RO.place_poses(centres, rng, NF)
        self.x[1], self.z[1], self.a[1] = self.x[0], self.z[0], self.a[0]
        orend = OC.OracleRender(BR.FIXTURE_TILES)
        gray, _, rgb = orend.render(self.x, self.z, self.a)
        self.obj = np.concatenate([self.mask(i, self.t[i]) for i in range(NF)])
        home = np.concatenate([self.mask(i, 0) for i in range(NF)])
        self.rgb = rgb.copy()
        self.rgb[self.obj] = RO.RED
        self.masks = orend.line_detect(self.rgb[..., ::-1])
        self.gray = gray.copy()
        self.gray[self.obj] = RO.RED_GRAY
        # not vacuous: most frames show a bot away from home, and time alone changes a frame
        away = (self.obj != home).reshape(NF, -1).any(1)
        assert away.mean() >= 0.5, away.mean()
        assert self.obj.reshape(NF, -1).any(1).mean() >= 0.8
        assert not np.array_equal(self.obj[0], self.obj[1]) and self.t[0] != self.t[1]

    def records(self, t):
        tab = self.table.copy()
        tab[self.rows] = self.recs[min(int(t), ROWS - 1)]
        return tab

    def mask(self, i, t):
        return RO.object_mask(self.records(t), self.x[i], self.z[i], self.a[i])

    def pose(self, dev):
        return torch.from_numpy(np.ascontiguousarray(np.stack([self.x, self.z, self.a]))).to(dev)


@pytest.fixture(scope='module')
def scene(map_path, dev_path):
    return Scene(map_path, dev_path)


@pytest.mark.parametrize('frames', ['gray', 'index'])
def test_frames_match_composed_oracle(gpu, scene, map_path, frames):
    from aido1_amd.render import RenderOutput, decode_index
    env = make_env(map_path, NF, draw=True)
    env.reset()
    env.set_state(step_count=scene.t)
    out = RenderOutput(NF, gpu, slots=1, rgb=True, frames=frames)
    env.render_into(out, pose=scene.pose(gpu))
    torch.cuda.synchronize()
    assert np.array_equal(out.rgb.cpu().numpy(), scene.rgb)
    assert np.array_equal(out.masks.cpu().numpy(), scene.masks)
    ring = out.ring[:, 0]
    if ring.dtype == torch.uint8:
        assert np.array_equal(ring.cpu().numpy() == RO.PAL_RED, scene.obj)
        ring = decode_index(ring)
    assert np.array_equal(ring.cpu().numpy(), scene.gray)


def test_first_frame_after_a_respawn_shows_the_bots_home(gpu, map_path):
    """The render reads step_count as the decision left it: 0 after an
    auto-reset -- and the next decision meets the bots from home again."""
    from aido1_amd.render import RenderOutput
    n = 8
    env = make_env(map_path, n, draw=True)
    env.reset()
    w = env.map.bots[0]                          # every env looks at bot 0's home
    px, pz = RO.pose_seeing(w.pos[0], w.pos[2], 0.3, 0.5, 0.1)
    pose = torch.tensor([[px] * n, [pz] * n, [0.3] * n], dtype=torch.float64, device=gpu)
    shots = [RenderOutput(n, gpu, slots=1, rgb=True) for _ in range(3)]
    env.render_into(shots[0], pose=pose)                       # step_count 0: at home
    env.set_state(step_count=np.full(n, 60, np.uint32), env_step=np.full(n, 5000, np.uint32))
    env.render_into(shots[1], pose=pose)                       # 60 steps down the lane
    env.step_into(torch.zeros(n, 2, device=gpu))       # env_step > max_env_steps: all respawn
    torch.cuda.synchronize()
    assert env.out.done.all() and (env.get_state()['step_count'] == 0).all()
    env.render_into(shots[2], pose=pose)
    torch.cuda.synchronize()
    red = [(sh.rgb == torch.tensor(RO.RED, dtype=torch.uint8, device=gpu)).all(-1) for sh in shots]
    assert red[0].any() and not torch.equal(red[0], red[1])
    assert torch.equal(shots[2].rgb, shots[0].rgb)


def test_grouped_renders_are_refused(gpu, map_path):
    from aido1_amd._lib import DtError
    from aido1_amd.render import RenderOutput, render_group_into
    env = make_env(map_path, 8, draw=True)
    env.reset()
    out = RenderOutput(8, gpu, slots=3)
    pose = [torch.zeros(3, 8, dtype=torch.float64, device=gpu) for _ in range(3)]
    fresh = [torch.zeros(8, dtype=torch.uint8, device=gpu) for _ in range(3)]
    for k in (2, 3):
        extra = [torch.zeros_like(out.masks) for _ in range(k - 1)]
        with pytest.raises(DtError, match='bots'):
            render_group_into(env, out, extra, fresh[:k], pose[:k])
    assert env._L.dt_render_bots(env._h, None, None, 0, 0) == 0    # off: the group renders again
    render_group_into(env, out, [torch.zeros_like(out.masks)], fresh[:2], pose[:2])
    torch.cuda.synchronize()


class MixedScene:
    """32 poses around the walker and the bots of the mixed map where their
    env's step count puts them: the walker's corner 0 moved in float32
    (tests/test_gpu_walkers.py's rule), the bots' records from the table."""

    def __init__(self, path, dev_path):
        from aido1_amd.maps import load_map
        m = load_map(path, lane_bots=True)
        self.n = 32
        self.table, self.walk = m.render_table, m.render_walker_table
        self.rows = m.bot_render_rows
        assert list(self.rows) == [0, 3] and self.walk[1, 3] >= 1 and not self.walk[[0, 2, 3]].any()
        self.recs = m.bot_render_records(dev_path)
        rng = np.random.default_rng(22)
        self.t = rng.integers(0, MROWS, self.n).astype(np.uint32)
        w = m.objects[1]
        centres = []
        for i in range(self.n):
            if i % 2:
                centres.append(tuple(dev_path[int(self.t[i]), (i // 2) % 2, :2]))
            else:
                idx = WR.index_at(int(self.t[i]), w.W, w.K)
                centres.append((w.pos[0] + idx * w.vel * w.heading[0],
                                w.pos[2] + idx * w.vel * w.heading[1]))
        self.x, self.z, self.a = RO.place_poses(centres, rng, self.n)
        orend = OC.OracleRender(BR.FIXTURE_TILES)
        _, _, rgb = orend.render(self.x, self.z, self.a)
        self.obj = np.concatenate([self.mask(i, self.t[i]) for i in range(self.n)])
        home = np.concatenate([self.mask(i, 0) for i in range(self.n)])
        self.rgb = rgb.copy()
        self.rgb[self.obj] = RO.RED
        self.masks = orend.line_detect(self.rgb[..., ::-1])
        away = (self.obj != home).reshape(self.n, -1).any(1)
        assert away[0::2].mean() >= 0.4 and away[1::2].mean() >= 0.4, away

    def records(self, t):
        tab = self.table.copy()
        for j, (wx, wz, W, K) in enumerate(self.walk):
            if K != 0:
                idx = F(WR.index_at(int(t), int(W), int(K)))
                tab[j, 0] = tab[j, 0] + idx * wx
                tab[j, 1] = tab[j, 1] + idx * wz
        tab[self.rows] = self.recs[min(int(t), MROWS - 1)]
        assert tab.dtype == F
        return tab

    def mask(self, i, t):
        return RO.object_mask(self.records(t), self.x[i], self.z[i], self.a[i])


def test_frames_with_a_walker_and_bots(gpu, mixed_path, mixed_dev_path):
    """draw_objects on the mixed map: the kObj = 2 kernels with the walker
    table set too."""
    from aido1_amd.render import RenderOutput
    sc = MixedScene(mixed_path, mixed_dev_path)
    env = make_env(mixed_path, sc.n, draw=True, bot_rows=MROWS)
    env.reset()
    env.set_state(step_count=sc.t)
    out = RenderOutput(sc.n, gpu, slots=1, rgb=True, frames='index')
    pose = torch.from_numpy(np.ascontiguousarray(np.stack([sc.x, sc.z, sc.a]))).to(gpu)
    env.render_into(out, pose=pose)
    torch.cuda.synchronize()
    assert np.array_equal(out.rgb.cpu().numpy(), sc.rgb)
    assert np.array_equal(out.masks.cpu().numpy(), sc.masks)
    assert np.array_equal(out.ring[:, 0].cpu().numpy() == RO.PAL_RED, sc.obj)
    # a render walker's record cannot become a bot's, nor a bot's a walker's
    L, h = env._L, env._h
    rec = np.ascontiguousarray(env.map.bot_render_records(mixed_dev_path))
    assert L.dt_render_bots(h, ptr(rec), ptr(np.array([0, 1], np.int32)), MROWS, 2) == -1
    assert 'render walker' in _err(env) and 'bot 1' in _err(env), _err(env)
    wt = env.map.render_walker_table.copy()
    wt[3] = wt[1]
    assert L.dt_render_walkers(h, ptr(wt), 4) == -1 and 'render bot' in _err(env), _err(env)
    assert L.dt_render_walkers(h, ptr(env.map.render_walker_table.copy()), 4) == 0
    out2 = RenderOutput(sc.n, gpu, slots=1, rgb=True, frames='index')
    env.render_into(out2, pose=pose)
    torch.cuda.synchronize()
    assert torch.equal(out2.rgb, out.rgb)           # the refusals changed nothing
    env.check()


# ---- argument checks --------------------------------------------------------------------
def same_steps(a, b, gpu, dec=3):
    rng = np.random.default_rng(5)
    for _ in range(dec):
        act = torch.from_numpy(rng.uniform(0.3, 1.0, (a.n, 2)).astype(F)).to(gpu)
        oa, ob = a.step_into(act), b.step_into(act)
        torch.cuda.synchronize()
        assert torch.equal(oa.reward, ob.reward) and torch.equal(oa.done, ob.done)
    a.check()
    b.check()


def test_bot_path_argument_checks(gpu, map_path, dev_path):
    env = make_env(map_path, 8)
    L, h = env._L, env._h
    home, par = env.map.bot_home.copy(), env.map.bot_param_table.copy()
    out = np.full((20, 3, 3), -7.0)

    def call(home=home, par=par, n=3, rows=20, out=out):
        return L.dt_bot_path(h, None if home is None else ptr(np.ascontiguousarray(home)),
                             None if par is None else ptr(np.ascontiguousarray(par)), n, rows,
                             None if out is None else ptr(out))
    assert call() == 0 and np.array_equal(out, dev_path[:20])
    out[:] = -7.0
    for kw, msg in ((dict(n=0), 'n must be'), (dict(n=257), 'n must be'),
                    (dict(rows=0), 'rows in'), (dict(rows=131073), 'rows in'),
                    (dict(home=None), 'required'), (dict(par=None), 'required'),
                    (dict(out=None), 'required')):
        assert call(**kw) == -1 and msg in _err(env), (kw, _err(env))
    for (i, j), val, msg in (((1, 0), -0.1, 'velocity >= 0'), ((1, 1), 0.0, 'follow_dist > 0'),
                             ((1, 4), 0.0, 'radius > 0'), ((1, 5), -27.0, 'k > 0'),
                             ((1, 6), -1.0, 'limit >= 0'), ((1, 2), np.nan, 'non-finite'),
                             ((1, 1), np.inf, 'non-finite')):
        bad = par.copy()
        bad[i, j] = val
        assert call(par=bad) == -1 and msg in _err(env) and 'bot 1' in _err(env), _err(env)
    bad = home.copy()
    bad[2, 2] = np.nan
    assert call(home=bad) == -1 and 'non-finite' in _err(env) and 'bot 2' in _err(env)
    # an undefined path: bot 1 starts on the grass tile
    bad = home.copy()
    bad[1, :2] = 0.61 * 1.5
    assert call(home=bad) == -1
    assert 'bot 1, step 1' in _err(env) and 'drivable' in _err(env), _err(env)
    assert (out == -7.0).all()               # nothing was written
    # the path's own byte cap, checked before anything is read: 131072 x 100 x 24 B
    assert call(home=np.zeros((100, 3)), par=np.zeros((100, 7)), n=100, rows=131072) == -1
    assert 'is over' in _err(env), _err(env)
    assert call() == 0 and np.array_equal(out, dev_path[:20])
    fresh = make_env(map_path, 8)
    env.reset()
    fresh.reset()
    same_steps(env, fresh, gpu)


def test_path_across_a_chunk_boundary(gpu, map_path):
    """8200 rows: the second launch takes row 8192 of the first as its input.
    The rows around the hand-over, one step at a time as above."""
    env = make_env(map_path, 8, bot_rows=8)
    rows = 8200
    home = np.ascontiguousarray(env.map.bot_home)
    par = np.ascontiguousarray(env.map.bot_param_table)
    path = np.zeros((rows, 3, 3))
    assert env._L.dt_bot_path(env._h, ptr(home), ptr(par), 3, rows, ptr(path)) == 0, _err(env)
    sim = R.SimulatorRef(BR.FIXTURE_TILES)
    bots = [BR.Bot(d, 0.61) for d in BR.split_objects(BR.FIXTURE_OBJECTS)[1]]
    for b, bot in enumerate(bots):
        for t in list(range(8186, rows - 1)) + [0, 4000]:
            want = BR.bot_step(sim, *path[t, b], bot.velocity, bot.follow_dist)
            assert np.max(np.abs(np.array(want) - path[t + 1, b])) <= TOL, (b, t)
    assert np.isfinite(path).all() and (np.abs(np.diff(path[8185:8199, :, :2], axis=0)) > 0).any()


def test_set_bots_argument_checks(gpu, map_path, dev_path, tmp_path):
    env = make_env(map_path, 8, bot_rows=32)
    L, h = env._L, env._h
    rec = np.ascontiguousarray(env.map.bot_records(dev_path[:32]))
    row = np.ascontiguousarray(env.map.bot_object_rows, np.int32)
    assert list(row) == [1, 2, 3]

    def call(rec=rec, row=row, rows=32, n=3):
        return L.dt_set_bots(h, None if rec is None else ptr(rec),
                             None if row is None else ptr(np.ascontiguousarray(row, np.int32)),
                             rows, n)
    assert call() == 0
    for kw, msg in ((dict(rows=0), 'rows must be'), (dict(rows=131073), 'rows must be'),
                    (dict(n=-1), 'n must be'), (dict(n=5), 'n must be'),
                    (dict(rec=None), 'required'), (dict(row=None), 'required'),
                    (dict(row=[1, 2, 4]), 'outside'), (dict(row=[1, -1, 3]), 'outside'),
                    (dict(row=[1, 2, 1]), 'twice')):
        assert call(**kw) == -1 and msg in _err(env), (kw, _err(env))
    for val in (np.nan, np.inf):
        bad = rec.copy()
        bad[17, 1, 5] = val
        assert call(rec=bad) == -1 and 'non-finite' in _err(env) and 'row 17' in _err(env)
    # the refusals changed nothing: the env steps as a fresh one does
    fresh = make_env(map_path, 8, bot_rows=32)
    env.reset()
    fresh.reset()
    same_steps(env, fresh, gpu)
    # n = 0 switches the bots off (they stand at home as static objects), and on again
    assert call(n=0) == 0 and call() == 0
    env.close()
    # an index naming a walker row, and a walker on a bot's row
    objs = [dict(WR.DUCKIE, pos=[1.5, 0.05], rotate=-90, static=False, wait=0.1),
            dict(BR.BOT, pos=[0.3, 1.5], rotate=-90)]
    mixed = make_env(BR.write_map(tmp_path / 'mixed.yaml', objs), 8, bot_rows=32)
    assert mixed.map.has_walkers and list(mixed.map.bot_object_rows) == [1]
    rec1 = np.ascontiguousarray(mixed.map.bot_records(mixed.bot_path))
    assert mixed._L.dt_set_bots(mixed._h, ptr(rec1), ptr(np.array([0], np.int32)), 32, 1) == -1
    assert 'walker' in _err(mixed)
    wt = mixed.map.walker_table.copy()
    wt[1] = wt[0]
    assert mixed._L.dt_set_walkers(mixed._h, ptr(wt), 2) == -1 and 'bot' in _err(mixed)
    mixed.reset()
    mixed.step_into(torch.full((8, 2), 0.5, device=gpu))
    mixed.check()
    mixed.close()
    # the byte cap: 14 collidable rows x 131072 table rows x 160 B > 256 MB
    # (refused before recs is read: a small buffer stands in)
    cones = [dict(kind='cone', pos=[0.3 + 0.25 * i, 0.3], height=0.1,
                  mesh_min=[-0.35, 0.0, -0.35], mesh_max=[0.35, 1.0, 0.35]) for i in range(14)]
    big = make_env(BR.write_map(tmp_path / 'cones.yaml', cones), 8, lane_bots=False)
    assert len(big.map.object_table) == 14
    small = np.zeros(20)
    rows14 = np.arange(14, dtype=np.int32)
    assert big._L.dt_set_bots(big._h, ptr(small), ptr(rows14), 131072, 14) == -1
    assert 'is over' in _err(big)
    big.close()


def test_render_bots_argument_checks(gpu, map_path, dev_path):
    env = make_env(map_path, 8, draw=True, bot_rows=32)
    L, h = env._L, env._h
    rec = np.ascontiguousarray(env.map.bot_render_records(dev_path[:32]))
    row = np.ascontiguousarray(env.map.bot_render_rows, np.int32)
    assert list(row) == [0, 2, 3] and rec.shape == (32, 3, 8)

    def call(rec=rec, row=row, rows=32, n=3):
        return L.dt_render_bots(h, None if rec is None else ptr(rec),
                                None if row is None else ptr(np.ascontiguousarray(row, np.int32)),
                                rows, n)
    assert call() == 0
    for kw, msg in ((dict(rows=0), 'rows must be'), (dict(rows=131073), 'rows must be'),
                    (dict(n=-1), 'n must be'), (dict(n=5), 'n must be'),
                    (dict(rec=None), 'required'), (dict(row=None), 'required'),
                    (dict(row=[0, 2, 4]), 'outside'), (dict(row=[0, -1, 3]), 'outside'),
                    (dict(row=[0, 2, 0]), 'twice')):
        assert call(**kw) == -1 and msg in _err(env), (kw, _err(env))
    bad = rec.copy()
    bad[9, 2, 0] = np.nan
    assert call(rec=bad) == -1 and 'non-finite' in _err(env) and 'row 9' in _err(env)
    # the byte cap, refused before recs is read (a small buffer stands in):
    # 65 records x 131072 rows x 32 B > 256 MB
    many = np.zeros((65, 8), F)
    many[:, 6:] = 1.0
    assert L.dt_render_objects(h, ptr(many), 65) == 0
    assert L.dt_render_bots(h, ptr(np.zeros(8, F)), ptr(np.arange(65, dtype=np.int32)),
                            131072, 65) == -1 and 'is over' in _err(env), _err(env)
    tab = np.ascontiguousarray(env.map.render_table, F)
    assert L.dt_render_objects(h, ptr(tab), len(tab)) == 0 and call() == 0
    # nothing changed: the frame is a fresh handle's
    from aido1_amd.render import RenderOutput
    fresh = make_env(map_path, 8, draw=True, bot_rows=32)
    t = np.arange(8, dtype=np.uint32) * 4
    w = env.map.bots[0]
    px, pz = RO.pose_seeing(w.pos[0], w.pos[2], 0.3, 0.5, 0.1)
    pose = torch.tensor([[px] * 8, [pz] * 8, [0.3] * 8], dtype=torch.float64, device=gpu)
    shots = []
    for e in (env, fresh):
        e.reset()
        e.set_state(step_count=t)
        out = RenderOutput(8, gpu, slots=1, rgb=True)
        e.render_into(out, pose=pose)
        torch.cuda.synchronize()
        shots.append(out.rgb.clone())
    assert torch.equal(shots[0], shots[1])
    assert not torch.equal(shots[0][0], shots[0][7])       # the bot moved in the frame


def test_vec_env_refuses_a_table_too_large(gpu, map_path):
    with pytest.raises(ValueError, match='bot_rows='):
        make_env(map_path, 8, bot_rows=None, max_steps=500001, max_env_steps=200000)
    with pytest.raises(ValueError, match='max_env_steps'):
        make_env(map_path, 8, bot_rows=131073)
    from aido1_amd.config import EnvConfig
    from aido1_amd.vec_env import VecEnv
    with pytest.raises(NotImplementedError, match='lane_bots'):
        VecEnv(8, config=EnvConfig(map_name=map_path))


# ---- the layers above VecEnv ------------------------------------------------------------
def test_host_layers_load_loop_dyn_duckiebots(gpu):
    """Simulator, launch_env, the env server's batch and ActorRollout get the
    bots through VecEnv: each loads the shipped map, steps and renders it."""
    from conftest import golden
    from aido1_amd.env import launch_env
    from aido1_amd.env_server import GpuBatch
    from aido1_amd.rollout import ActorRollout
    from aido1_amd.simulator import Simulator
    MAP = 'loop_dyn_duckiebots'
    # (the Simulator alone has no wrapper to bound an episode: max_steps = 500001
    # rows would be over the cap, so the table's size is given)
    for sim in (Simulator(seed=3, map_name=MAP, device=0, draw_objects=True, lane_bots=True,
                          bot_rows=2002, accept_start_angle_deg=4),
                launch_env(device=0, map_name=MAP, lane_bots=True, bot_rows=2002)):
        assert len(sim._env.map.bots) == 3 and sim._env.bot_path.shape == (2002, 3, 3)
        obs = sim.reset()
        obs, reward, done, _ = sim.step(np.array([0.4, 0.4]))
        assert obs.shape == (120, 160, 3) and np.isfinite(reward)
        sim._env.check()
    with pytest.raises(ValueError, match='bot_rows='):
        Simulator(seed=3, map_name=MAP, device=0, lane_bots=True)
    batch = GpuBatch(4, map_name=MAP, device=0, draw_objects=True, lane_bots=True, max_steps=1500)
    assert len(batch.env.map.bots) == 3
    batch.reset([0, 1, 2, 3])
    batch.step([0, 2], np.full((2, 2), 0.5, np.float32))
    batch.env.check()
    torch.manual_seed(1)
    roll = ActorRollout(golden('reference_config.json'), 16, maps=(MAP,), device=0, seed=21,
                        frames='index', draw_objects=True, lane_bots=True)
    assert len(roll.envs[0].map.bots) == 3 and roll.envs[0].draw_objects
    roll.reset()
    for _ in range(3):
        roll.step()
    torch.cuda.synchronize()
    assert (roll.envs[0].get_state()['step_count'] > 0).any()
    assert roll.envs[0].check() == 0
    roll.close()
