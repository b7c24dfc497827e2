"""GPU: walkers (dt_set_walkers / dt_render_walkers) in both step kernels and
the render's object phase, against the CPU restatement of tests/walkers_ref.py
(steps: done and tile exact, rewards within 1e-9, the project's bound for GPU
against oracle, tests/test_gpu_step.py) and tests/render_objects_ref.py's
composition with each env's shifted table (frames: bit for bit)."""
import ctypes

import numpy as np
import pytest
import torch

import render_objects_ref as RO
import walkers_ref as WR
from oracle import dtsim_ref as R
from oracle import oracle_c as OC

pytestmark = pytest.mark.gpu

TOL = 1e-9
SEED = 2024
N, DEC, K_MANY = 96, 40, 8     # six fan workgroups / a partial step_kernel block
F = np.float32


@pytest.fixture(scope='module')
def map_path(tmp_path_factory):
    return WR.write_map(tmp_path_factory.mktemp('walkers') / 'walkers.yaml')


@pytest.fixture(scope='module')
def static_path(tmp_path_factory):
    return WR.write_map(tmp_path_factory.mktemp('walkers') / 'static_twin.yaml',
                        WR.all_static(WR.FIXTURE_OBJECTS))


def make_env(path, n, seed=SEED, draw=False, **cfg_kw):
    from aido1_amd.config import EnvConfig
    from aido1_amd.vec_env import VecEnv
    return VecEnv(n, seed=seed, config=EnvConfig(map_name=path, **cfg_kw), draw_objects=draw)


class Run:
    """The restatement's run: n envs reset, every step_count set to U{0..199},
    `dec` decisions of actions U[0.3, 1)^2.  Computed once, never changed."""

    def __init__(self, n, dec, rng_seed, **cfg_kw):
        rng = np.random.default_rng(rng_seed)
        self.n, self.dec, self.cfg_kw = n, dec, cfg_kw
        self.ref = WR.WalkerBatchRef(WR.FIXTURE_TILES, WR.FIXTURE_OBJECTS, n, SEED, **cfg_kw)
        self.ref.reset()
        self.start = self.ref.state()
        self.t0 = rng.integers(0, 200, n).astype(np.uint32)
        self.ref.set_step_count(self.t0)
        self.actions = rng.uniform(0.3, 1.0, (dec, n, 2)).astype(F)
        self.outs = [self.ref.step(self.actions[d]) for d in range(dec)]
        self.end = self.ref.state()

    def fresh_env(self, path):
        env = make_env(path, self.n, **self.cfg_kw)
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


@pytest.fixture(scope='module')
def run():
    r = Run(N, DEC, 7)
    # not vacuous, on the restatement's own results: walkers away from home end
    # episodes, and the penalty is at work
    ref = r.ref
    print('episode ends %d, of them walker hits away from home %d; decisions %d, negative '
          'penalty %d' % (ref.ends, ref.walker_ends, ref.decisions, ref.negative))
    assert ref.walker_ends >= 0.05 * ref.ends > 0
    assert ref.negative >= 0.05 * ref.decisions
    return r


def test_step_parity_step_kernel(gpu, run, map_path):
    """dt_step: step_kernel's walker instantiation, a partial block."""
    env = run.fresh_env(map_path)
    for d in range(run.dec):
        out = env.step_into(torch.from_numpy(run.actions[d]).to(gpu))
        torch.cuda.synchronize()
        run.check(d, out.reward.cpu().numpy(), out.reward_mod.cpu().numpy(),
                  out.done.cpu().numpy(), out.tile.cpu().numpy())
    run.check_end(env)


def test_step_parity_fan_kernel(gpu, run, map_path):
    """dt_step_many at k = 8: step_fan_kernel's walker instantiation, wave 0
    testing the decision's three poses at t + 1, t + 2, t + 3."""
    from aido1_amd.vec_env import StepOutput
    env = run.fresh_env(map_path)
    out = StepOutput(K_MANY * N, gpu, lanepos=False, tile=False)
    for d0 in range(0, run.dec, K_MANY):
        a = torch.from_numpy(np.ascontiguousarray(run.actions[d0:d0 + K_MANY])).to(gpu)
        env.step_many_into(a, out)
        torch.cuda.synchronize()
        r, rm, dn = (t.cpu().numpy().reshape(K_MANY, N)
                     for t in (out.reward, out.reward_mod, out.done))
        for i in range(K_MANY):
            run.check(d0 + i, r[i], rm[i], dn[i])
    run.check_end(env)


def test_step_many_generic_path(gpu, map_path):
    """repeat 4 x frame_skip 2 = 8 Simulator steps a decision: dt_step_many runs
    step_kernel over the k decisions, the walkers at the counter after both
    increments of a Simulator.step."""
    from aido1_amd.vec_env import StepOutput
    n, dec = 32, 10
    r = Run(n, dec, 9, repeat_actions=4, frame_skip=2)
    assert r.ref.ends > 0 and r.ref.negative > 0
    env = r.fresh_env(map_path)
    out = StepOutput(dec * n, gpu, lanepos=False, tile=False)
    env.step_many_into(torch.from_numpy(r.actions).to(gpu), out)
    torch.cuda.synchronize()
    rw, rm, dn = (t.cpu().numpy().reshape(dec, n) for t in (out.reward, out.reward_mod, out.done))
    for d in range(dec):
        r.check(d, rw[d], rm[d], dn[d])
    r.check_end(env)


def test_leg_boundaries(gpu, map_path):
    """step_count injected at W - 2 .. W + 1, P - 2 .. P + 1 and 2P - 2 .. 2P + 1
    of each walker, so the three steps of one decision straddle every switch
    (wait -> walk, arrive -> wait, home again); the agent stands still 2 cm
    ahead of where the walker is a step later."""
    from aido1_amd.vec_env import StepOutput
    probe = WR.WalkerSimRef(WR.FIXTURE_TILES, objects=WR.FIXTURE_OBJECTS)
    off = R.CAMERA_FORWARD_DIST - R.ROBOT_LENGTH / 2
    ts, xs, zs, angs = [], [], [], []
    for w in probe.walkers:
        P = w.W + w.K
        for base in (w.W, P, 2 * P):
            for o in (-2, -1, 0, 1):
                t = max(0, base + o)
                sign = 1.0 if ((t + 3) // P) % 2 == 0 else -1.0
                dx, dz = w.shift(t + 1)
                gap = 0.04 + 0.02 + R.ROBOT_LENGTH / 2     # walker half length, 2 cm, agent
                cx = w.pos[0] + dx + sign * w.hx * gap
                cz = w.pos[2] + dz + sign * w.hz * gap
                a = float(np.arctan2(-sign * w.hz, sign * w.hx))   # facing away from the walker
                ts.append(t)
                angs.append(a)
                xs.append(cx - off * np.cos(a))
                zs.append(cz - off * -np.sin(a))
    n = len(ts)
    assert n == 36
    ref = WR.WalkerBatchRef(WR.FIXTURE_TILES, WR.FIXTURE_OBJECTS, n, SEED)
    ref.reset()
    ref.set_pose(xs, zs, angs)
    ref.set_step_count(ts)
    zero = np.zeros((n, 2), F)
    want = ref.step(zero)
    assert 0 < want['done'].sum() < n, want['done']
    assert ref.walker_ends > 0 and ref.negative > 0
    for many in (False, True):
        env = make_env(map_path, n)
        env.reset()
        env.set_state(x=xs, z=zs, angle=angs, step_count=np.array(ts, np.uint32))
        if many:
            out = StepOutput(n, gpu, lanepos=False, tile=False)
            env.step_many_into(torch.from_numpy(zero[None]).to(gpu), out)
        else:
            out = env.step_into(torch.from_numpy(zero).to(gpu))
        torch.cuda.synchronize()
        assert np.array_equal(out.done.cpu().numpy(), want['done']), many
        assert np.max(np.abs(out.reward.cpu().numpy() - want['reward'])) <= TOL
        assert np.max(np.abs(out.reward_mod.cpu().numpy() - want['reward_mod'])) <= TOL
        env.check()


def test_graph_replay_equals_eager(gpu, run, map_path):
    """A captured graph of 6 dt_step launches replayed twice equals 12 eager
    steps: nothing about the walkers is decided on the host per launch."""
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


# ---- argument checks ------------------------------------------------------------------------
def _err(env):
    return env._L.dt_last_error(env._h).decode()


def test_set_walkers_argument_checks(gpu, map_path):
    env = make_env(map_path, 8)
    good = env.map.walker_table.copy()
    L, h = env._L, env._h

    def call(tab, n=None):
        tab = np.ascontiguousarray(tab, np.float64)
        return L.dt_set_walkers(h, tab.ctypes.data_as(ctypes.c_void_p),
                                len(tab) if n is None else n)
    assert len(good) == 4 and call(good) == 0
    for col, val, msg in ((0, np.nan, 'non-finite'), (2, np.inf, 'non-finite'),
                          (2, 0.0, 'vel must be > 0'), (2, -0.02, 'vel must be > 0'),
                          (4, 0.0, 'K must be >= 1'), (3, 2.5, 'whole numbers'),
                          (4, 7.25, 'whole numbers'), (3, -1.0, 'whole numbers'),
                          (4, 2.0 ** 24, 'whole numbers')):
        bad = good.copy()
        bad[2, col] = val
        assert call(bad) == -1, (col, val)
        assert msg in _err(env) and 'row 2' in _err(env), (_err(env), msg)
    assert call(good[:3]) == -1 and 'n must be 0 or' in _err(env)
    assert call(np.zeros((5, 5))) == -1 and 'n must be 0 or' in _err(env)
    assert L.dt_set_walkers(h, None, 4) == -1 and 'null' in _err(env)
    assert call(np.zeros((4, 5))) == 0 and call(good, 0) == 0 and call(good) == 0
    # a refused call changed nothing: the env still steps with its walkers
    env.reset()
    env.step_into(torch.zeros(8, 2, device=gpu))
    env.check()


def test_render_walkers_argument_checks(gpu, map_path):
    from aido1_amd._lib import DtError
    from aido1_amd.render import RenderOutput, render_group_into
    env = make_env(map_path, 8, draw=True)
    good = env.map.render_walker_table.copy()
    L, h = env._L, env._h

    def call(tab, n=None):
        tab = np.ascontiguousarray(tab, np.float32)
        return L.dt_render_walkers(h, tab.ctypes.data_as(ctypes.c_void_p),
                                   len(tab) if n is None else n)
    assert len(good) == 4 and call(good) == 0
    for col, val, msg in ((0, np.nan, 'non-finite'), (1, np.inf, 'non-finite'),
                          (3, 0.0, 'K must be >= 1'), (2, 2.5, 'whole numbers'),
                          (3, 7.25, 'whole numbers'), (2, -1.0, 'whole numbers')):
        bad = good.copy()
        bad[0, col] = val
        assert call(bad) == -1, (col, val)
        assert msg in _err(env) and 'row 0' in _err(env), (_err(env), msg)
    assert call(good[:3]) == -1 and 'n must be 0 or' in _err(env)
    assert L.dt_render_walkers(h, None, 4) == -1 and 'null' in _err(env)
    # a grouped launch has no step counter per decision: refused while walkers are drawn
    env.reset()
    out = RenderOutput(8, gpu, slots=3)
    pose = [torch.zeros(3, 8, dtype=torch.float64, device=gpu) for _ in range(3)]
    fresh = [torch.zeros(8, dtype=torch.uint8, device=gpu) for _ in range(3)]
    for k in (2, 3):
        extra = [torch.zeros_like(out.masks) for _ in range(k - 1)]
        with pytest.raises(DtError, match='render walkers'):
            render_group_into(env, out, extra, fresh[:k], pose[:k])
    assert call(good, 0) == 0      # off: the group renders again
    render_group_into(env, out, [torch.zeros_like(out.masks)], fresh[:2], pose[:2])
    torch.cuda.synchronize()


# ---- frames ---------------------------------------------------------------------------------
NF = 64


class Scene:
    """64 poses around the walkers where their env's step count puts them, and
    the expected frames: the oracle's object-free frame, each env's shifted
    footprints painted red, the oracle's line detector on that image."""

    def __init__(self, path):
        from aido1_amd.maps import load_map
        m = load_map(path)
        self.table, self.walk = m.render_table, m.render_walker_table
        rng = np.random.default_rng(21)
        walkers = [o for o in m.objects if o.walker]
        self.t = rng.integers(0, 2 * 2 * (3 + 44), NF).astype(np.uint32)   # two periods of walker 1
        self.t[1] = self.t[0] + 3 + 20          # env 1: env 0's pose at another time
        centres = []
        for i in range(NF):
            o = walkers[i % 3]
            idx = WR.index_at(int(self.t[i]), o.W, o.K)
            centres.append((o.pos[0] + idx * o.vel * o.heading[0],
                            o.pos[2] + idx * o.vel * o.heading[1]))
        self.x, self.z, self.a = RO.place_poses(centres, rng, NF)
        self.x[1], self.z[1], self.a[1] = self.x[0], self.z[0], self.a[0]
        orend = OC.OracleRender(WR.FIXTURE_TILES)
        gray, _, rgb = orend.render(self.x, self.z, self.a)
        self.obj = np.concatenate([self.mask(i, self.t[i]) for i in range(NF)])
        home = np.concatenate([self.mask(i, 0) for i in range(NF)])
        self.rgb = rgb.copy()
        self.rgb[self.obj] = RO.RED
        self.masks = orend.line_detect(self.rgb[..., ::-1])
        self.gray = gray.copy()
        self.gray[self.obj] = RO.RED_GRAY
        # not vacuous: most frames show a walker away from home, and time alone changes a frame
        away = (self.obj != home).reshape(NF, -1).any(1)
        assert away.mean() >= 0.5, away.mean()
        assert self.obj.reshape(NF, -1).any(1).mean() >= 0.8
        assert not np.array_equal(self.obj[0], self.obj[1]) and self.t[0] != self.t[1]

    def shifted(self, t):
        """The records at step count t: corner 0 moved in float32, one product
        and one sum each (numpy float32 never contracts)."""
        tab = self.table.copy()
        for j, (wx, wz, W, K) in enumerate(self.walk):
            if K == 0:
                continue
            idx = F(WR.index_at(int(t), int(W), int(K)))
            tab[j, 0] = tab[j, 0] + idx * wx
            tab[j, 1] = tab[j, 1] + idx * wz
        assert tab.dtype == F
        return tab

    def mask(self, i, t):
        return RO.object_mask(self.shifted(t), self.x[i], self.z[i], self.a[i])

    def pose(self, dev):
        return torch.from_numpy(np.ascontiguousarray(np.stack([self.x, self.z, self.a]))).to(dev)


@pytest.fixture(scope='module')
def scene(map_path):
    return Scene(map_path)


@pytest.mark.parametrize('list_cap', [0, 64], ids=['lds', 'spill'])
@pytest.mark.parametrize('frames', ['gray', 'index'])
def test_frames_match_composed_oracle(gpu, scene, map_path, frames, list_cap):
    from aido1_amd.render import RenderOutput, decode_index
    env = make_env(map_path, NF, draw=True)
    env.reset()
    env.set_state(step_count=scene.t)
    out = RenderOutput(NF, gpu, slots=1, rgb=True, frames=frames)
    env.render_into(out, pose=scene.pose(gpu), list_cap=list_cap)
    torch.cuda.synchronize()
    assert np.array_equal(out.rgb.cpu().numpy(), scene.rgb)
    assert np.array_equal(out.masks.cpu().numpy(), scene.masks)
    ring = out.ring[:, 0]
    if ring.dtype == torch.uint8:
        assert np.array_equal(ring.cpu().numpy() == RO.PAL_RED, scene.obj)
        ring = decode_index(ring)
    assert np.array_equal(ring.cpu().numpy(), scene.gray)


def test_first_frame_after_a_respawn_shows_the_walkers_home(gpu, map_path):
    """The render reads step_count as the decision left it: 0 after an auto-reset."""
    from aido1_amd.render import RenderOutput
    n = 8
    env = make_env(map_path, n, draw=True)
    env.reset()
    w = env.map.objects[0]                       # every env looks at walker 1's home
    px, pz = RO.pose_seeing(w.pos[0], w.pos[2], 0.3, 0.5, 0.1)
    pose = torch.tensor([[px] * n, [pz] * n, [0.3] * n], dtype=torch.float64, device=gpu)
    shots = [RenderOutput(n, gpu, slots=1, rgb=True) for _ in range(3)]
    env.render_into(shots[0], pose=pose)                       # step_count 0: at home
    env.set_state(step_count=np.full(n, 30, np.uint32), env_step=np.full(n, 5000, np.uint32))
    env.render_into(shots[1], pose=pose)                       # 27 steps from home
    env.step_into(torch.zeros(n, 2, device=gpu))       # env_step > max_env_steps: all respawn
    torch.cuda.synchronize()
    assert env.out.done.all() and (env.get_state()['step_count'] == 0).all()
    env.render_into(shots[2], pose=pose)
    torch.cuda.synchronize()
    red = [(sh.rgb == torch.tensor(RO.RED, dtype=torch.uint8, device=gpu)).all(-1) for sh in shots]
    assert red[0].any() and not torch.equal(red[0], red[1])
    assert torch.equal(shots[2].rgb, shots[0].rgb)


# ---- unchanged when off ---------------------------------------------------------------------
def test_all_zero_rows_change_nothing(gpu, scene, static_path):
    """The all-static twin: no walker upload (the kernels as they were) against
    an upload of all-zero rows (the walker instantiations, every row static),
    bit for bit in steps and frames."""
    from aido1_amd.render import RenderOutput
    from aido1_amd.vec_env import StepOutput
    n, dec = NF, 12
    rng = np.random.default_rng(4)
    acts = torch.from_numpy(rng.uniform(0.3, 1.0, (dec, n, 2)).astype(F)).to(gpu)
    results = []
    for upload in (False, True):
        env = make_env(static_path, n, draw=True)
        assert not env.map.has_walkers and len(env.map.object_table) == 4
        if upload:
            z64, z32 = np.zeros((4, 5)), np.zeros((4, 4), F)
            assert env._L.dt_set_walkers(env._h, z64.ctypes.data_as(ctypes.c_void_p), 4) == 0
            assert env._L.dt_render_walkers(env._h, z32.ctypes.data_as(ctypes.c_void_p), 4) == 0
        env.reset()
        env.set_state(step_count=scene.t)
        res = []
        for d in range(4):
            o = env.step_into(acts[d])
            res += [o.reward.clone(), o.reward_mod.clone(), o.done.clone(), o.tile.clone()]
        many = StepOutput((dec - 4) * n, gpu, lanepos=False, tile=False)
        env.step_many_into(acts[4:].contiguous(), many)
        res += [many.reward, many.reward_mod, many.done]
        for frames in ('gray', 'index'):
            out = RenderOutput(n, gpu, slots=1, rgb=True, frames=frames)
            env.render_into(out, pose=scene.pose(gpu))
            res += [out.rgb, out.masks, out.ring]
        torch.cuda.synchronize()
        env.check()
        st = env.get_state()
        res += [torch.from_numpy(st[k]) for k in sorted(st)]
        results.append(res)
    assert len(results[0]) == len(results[1])
    for i, (a, b) in enumerate(zip(*results)):
        assert torch.equal(a, b), i
    assert any(bool(r.any()) for r in results[0][2:16:4])    # some episode ended


# ---- the layers above VecEnv ---------------------------------------------------------------
def test_host_layers_load_loop_pedestrians(gpu):
    """Simulator, launch_env, the env server's batch and ActorRollout get the
    walkers through VecEnv: each loads the shipped map, steps and renders it."""
    from conftest import golden
    from aido1_amd.env import launch_env
    from aido1_amd.env_server import GpuBatch
    from aido1_amd.rollout import ActorRollout
    from aido1_amd.simulator import Simulator
    MAP = 'loop_pedestrians'
    for sim in (Simulator(seed=3, map_name=MAP, device=0, draw_objects=True,
                          accept_start_angle_deg=4),
                launch_env(device=0, map_name=MAP)):
        assert sim._env.map.has_walkers
        obs = sim.reset()
        obs, reward, done, _ = sim.step(np.array([0.4, 0.4]))
        assert obs.shape == (120, 160, 3) and np.isfinite(reward)
        sim._env.check()
    batch = GpuBatch(4, map_name=MAP, device=0, draw_objects=True)
    assert batch.env.map.has_walkers
    batch.reset([0, 1, 2, 3])
    batch.step([0, 2], np.full((2, 2), 0.5, np.float32))
    batch.env.check()
    torch.manual_seed(1)
    roll = ActorRollout(golden('reference_config.json'), 16, maps=(MAP,), device=0, seed=21,
                        frames='index', draw_objects=True)
    assert roll.envs[0].map.has_walkers and roll.envs[0].draw_objects
    roll.reset()
    for _ in range(3):
        roll.step()
    torch.cuda.synchronize()
    assert (roll.envs[0].get_state()['step_count'] > 0).any()
    assert roll.envs[0].check() == 0
    roll.close()
