"""GPU: each decision's step counter travels with its pose -- dt_step_many_time's
time output, dt_copy_time beside dt_copy_pose, and dt_render_group's renders at
a given time (one decision: the snapshot render; two or three: the grouped
launch on a handle that draws walkers or bots).

Every comparison is bit for bit, and the expected side is always the existing
single-decision path (step_into, set_state(step_count=) + render_into) on the
same handle or on a twin with the same seed -- never the new path itself.
Maps, scenes and poses are the walker, bot and object tests' own."""
import ctypes

import numpy as np
import pytest
import torch

import bots_ref as BR
import test_gpu_bots as TB
import test_gpu_walkers as TW
import walkers_ref as WR

pytestmark = pytest.mark.gpu

F = np.float32
NF = 64
LIST_CAP = 64          # the walker frames test's small list_cap: the overflow path


# ---- maps and envs ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def maps(tmp_path_factory):
    d = tmp_path_factory.mktemp('render_time')
    return {'walkers': WR.write_map(d / 'walkers.yaml'),
            'bots': BR.write_map(d / 'bots.yaml'),
            'mixed': BR.write_map(d / 'mixed.yaml', BR.MIXED_OBJECTS),
            'static': WR.write_map(d / 'static.yaml', WR.all_static(WR.FIXTURE_OBJECTS)),
            'loop_empty': 'loop_empty'}


def make_env(maps, kind, n, draw=False, **cfg_kw):
    if kind == 'bots':
        return TB.make_env(maps[kind], n, draw=draw, **cfg_kw)
    if kind == 'mixed':
        return TB.make_env(maps[kind], n, draw=draw, bot_rows=TB.MROWS, **cfg_kw)
    return TW.make_env(maps[kind], n, draw=draw, **cfg_kw)


def start_pair(maps, kind, n, rng, draw=False, **cfg_kw):
    """Two handles in one state: reset, step counters U{1..199}, and on a
    quarter of the envs env_step at max_env_steps - {0, 1, 2}, so that those
    respawn in the first three decisions."""
    envs = [make_env(maps, kind, n, draw=draw, **cfg_kw) for _ in range(2)]
    t0 = rng.integers(1, 200, n).astype(np.uint32)
    es = np.zeros(n, np.uint32)
    es[::4] = envs[0].config.max_env_steps - (np.arange(0, n, 4) // 4) % 3
    for env in envs:
        env.reset()
        env.set_state(step_count=t0, env_step=es)
    a, b = envs[0].get_state(), envs[1].get_state()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    return envs[0], envs[1], t0


def u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- 1, 2: the time output ----------------------------------------------------------------
def check_chunk(gpu, maps, kind, n, k, rng_seed, **cfg_kw):
    """step_many_into(pose=, time=) against k step_into calls of the twin:
    time[d] is the twin's step_count after d + 1 calls, and rewards, done flags
    and poses are the twin's (nothing else moved)."""
    from aido1_amd.vec_env import StepOutput
    rng = np.random.default_rng(rng_seed)
    env, twin, t0 = start_pair(maps, kind, n, rng, **cfg_kw)
    acts = torch.from_numpy(rng.uniform(0.3, 1.0, (k, n, 2)).astype(F)).to(gpu)
    out = StepOutput(k * n, gpu, lanepos=False, tile=False)
    pose = torch.full((k, 3, n), np.nan, dtype=torch.float64, device=gpu)
    time = torch.full((k, n), -7, dtype=torch.int32, device=gpu)
    guard = torch.full((n,), -7, dtype=torch.int32, device=gpu)   # a canary allocated next
    env.step_many_into(acts, out, pose=pose, time=time)
    torch.cuda.synchronize()
    got_t = u32(time)
    rw, rm, dn = (t.cpu().numpy().reshape(k, n) for t in (out.reward, out.reward_mod, out.done))
    ob = out.obs.cpu().numpy().reshape(k, n, 2)
    ps = pose.cpu().numpy()
    prev, respawns = t0, 0
    for d in range(k):
        o = twin.step_into(acts[d])
        torch.cuda.synchronize()
        st = twin.get_state()
        assert np.array_equal(got_t[d], st['step_count']), (kind, d)
        assert np.array_equal(dn[d], o.done.cpu().numpy()), (kind, d)
        assert np.array_equal(rw[d], o.reward.cpu().numpy()), (kind, d)
        assert np.array_equal(rm[d], o.reward_mod.cpu().numpy()), (kind, d)
        assert np.array_equal(ob[d], o.obs.cpu().numpy()), (kind, d)
        for j, key in enumerate(('x', 'z', 'angle')):
            assert np.array_equal(ps[d, j], st[key]), (kind, d, key)
        respawns += int(((dn[d] != 0) & (got_t[d] == 0) & (prev != 0)).sum())
        prev = st['step_count']
    a, b = env.get_state(), twin.get_state()
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert (guard == -7).all()
    assert respawns > 0       # a time entry is 0 where the twin's counter before was not
    assert env.check() == 0 and twin.check() == 0


@pytest.mark.parametrize('kind', ['walkers', 'bots', 'mixed', 'loop_empty'])
def test_time_output_fan_path(gpu, maps, kind):
    """n = 40: two full fan workgroups and a half one; k = 8; the walker, bot
    (with a walker: mixed) and lean instantiations of step_fan_kernel."""
    check_chunk(gpu, maps, kind, 40, 8, 31)


def test_time_output_across_launches(gpu, maps):
    """k = 70 crosses kFanMaxK = 64: the second launch's outputs start at 64 n."""
    check_chunk(gpu, maps, 'walkers', 24, 70, 32)


def test_time_output_generic_path(gpu, maps):
    """repeat 4 x frame_skip 2: step_kernel a decision at a time, the counters
    copied after each launch."""
    check_chunk(gpu, maps, 'walkers', 24, 4, 33, repeat_actions=4, frame_skip=2)


def test_time_is_optional_and_checked(gpu, maps):
    """time=None is dt_step_many's call; a wrong time tensor is a ValueError."""
    from aido1_amd.vec_env import StepOutput
    n, k = 24, 3
    env = make_env(maps, 'walkers', n)
    env.reset()
    acts = torch.full((k, n, 2), 0.5, device=gpu)
    out = StepOutput(k * n, gpu, lanepos=False, tile=False)
    env.step_many_into(acts, out)
    for bad in (torch.zeros(k, n, dtype=torch.float32, device=gpu),
                torch.zeros(k, n + 1, dtype=torch.int32, device=gpu),
                torch.zeros(k + 1, n, dtype=torch.int32, device=gpu),
                torch.zeros(n, k, dtype=torch.int32, device=gpu).t(),
                torch.zeros(k, n, dtype=torch.int32)):
        with pytest.raises(ValueError, match='time'):
            env.step_many_into(acts, out, time=bad)
        with pytest.raises(ValueError, match='time'):
            env.bind_step_many(acts, out, time=bad)
    pose = torch.zeros(3, n, dtype=torch.float64, device=gpu)
    for bad in (torch.zeros(n, dtype=torch.int64, device=gpu),
                torch.zeros(n + 1, dtype=torch.int32, device=gpu),
                torch.zeros(n, dtype=torch.int32)):
        with pytest.raises(ValueError, match='time'):
            env.copy_pose(pose, time=bad)
    torch.cuda.synchronize()
    assert env.check() == 0


# ---- scenes -------------------------------------------------------------------------------
class Case:
    """A dynamic map's 64-frame scene (the walker and bot frame tests' own: its
    constructor asserts that most frames show an object away from home), a
    handle that draws it, and the times: the scene's (the bots' with their
    clamp cases), one entry set to 0 and one to 500000."""

    def __init__(self, maps, kind):
        self.kind = kind
        self.env = make_env(maps, kind, NF, draw=True)
        self.env.reset()
        if kind == 'bots':
            self.scene = TB.Scene(maps[kind], self.env.bot_path.copy())
            assert set([TB.ROWS - 1, TB.ROWS, TB.ROWS + 7, 500000]) <= set(self.scene.t.tolist())
            self.shift = 300
        else:
            self.scene = TW.Scene(maps[kind])
            self.shift = 3 + 20
        self.t = self.scene.t.copy()
        self.t[6], self.t[7] = 0, 500000
        self.other = (self.t + np.uint32(77)).astype(np.uint32)

    def dev_time(self, dev, t):
        return torch.from_numpy(np.ascontiguousarray(t).view(np.int32)).to(dev)


@pytest.fixture(scope='module', params=['walkers', 'bots'])
def case(request, gpu, maps):
    return Case(maps, request.param)


def outputs(out):
    return [t.clone() for t in (out.rgb, out.masks, out.ring) if t is not None]


# ---- 3: the snapshot render ---------------------------------------------------------------
@pytest.mark.parametrize('list_cap', [0, LIST_CAP], ids=['lds', 'spill'])
@pytest.mark.parametrize('frames', ['gray', 'index'])
def test_snapshot_render_at_a_given_time(gpu, case, frames, list_cap):
    """render_into(pose=P, time=T) with the handle's counters elsewhere equals
    set_state(step_count=T) + render_into(pose=P): rgb, masks and the ring."""
    from aido1_amd.render import RenderOutput
    env, pose = case.env, case.scene.pose(gpu)
    env.set_state(step_count=case.t)
    want = RenderOutput(NF, gpu, slots=1, rgb=True, frames=frames)
    env.render_into(want, pose=pose, list_cap=list_cap)
    env.set_state(step_count=case.other)
    moved = RenderOutput(NF, gpu, slots=1, rgb=True, frames=frames)
    env.render_into(moved, pose=pose, list_cap=list_cap)
    got = RenderOutput(NF, gpu, slots=1, rgb=True, frames=frames)
    env.render_into(got, pose=pose, list_cap=list_cap, time=case.dev_time(gpu, case.t))
    torch.cuda.synchronize()
    for a, b in zip(outputs(got), outputs(want)):
        assert torch.equal(a, b)
    assert not torch.equal(moved.rgb, want.rgb)      # the handle's own counters show another frame
    assert np.array_equal(env.get_state()['step_count'], case.other)   # and were not touched


def test_copy_pose_with_time_survives_the_next_step(gpu, case):
    """copy_pose(pose, time=), one more step_into, render_into(pose=, time=):
    the render taken before that step (bind_* forms alike)."""
    from aido1_amd.render import RenderOutput, bind_render
    env, sc = case.env, case.scene
    env.reset()
    env.set_state(x=sc.x, z=sc.z, angle=sc.a, step_count=case.t)
    want = RenderOutput(NF, gpu, slots=1, rgb=True)
    env.render_into(want)
    pose = torch.zeros(3, NF, dtype=torch.float64, device=gpu)
    time = torch.full((NF,), -1, dtype=torch.int32, device=gpu)
    env.copy_pose(pose, time=time)
    env.step_into(torch.full((NF, 2), 0.5, device=gpu))
    torch.cuda.synchronize()
    assert np.array_equal(u32(time), case.t)
    assert not np.array_equal(env.get_state()['step_count'], case.t)
    got, late, bound = (RenderOutput(NF, gpu, slots=1, rgb=True) for _ in range(3))
    env.render_into(got, pose=pose, time=time)
    env.render_into(late, pose=pose)                 # decision d's pose, d + 1's objects
    s = torch.cuda.current_stream(gpu)
    pose2, time2 = torch.zeros_like(pose), torch.zeros_like(time)
    assert bind_render(env, bound, s, pose=pose, time=time)() == 0
    assert env.bind_copy_pose(pose2, s, time=time2)() == 0
    torch.cuda.synchronize()
    for a, b in zip(outputs(got), outputs(want)):
        assert torch.equal(a, b)
    for a, b in zip(outputs(bound), outputs(want)):
        assert torch.equal(a, b)
    assert not torch.equal(late.rgb, want.rgb)
    st = env.get_state()
    assert np.array_equal(u32(time2), st['step_count'])
    assert np.array_equal(pose2.cpu().numpy(), np.stack([st['x'], st['z'], st['angle']]))


# ---- 4: the grouped render, times injected ------------------------------------------------
def injected(case, gpu):
    """Three decisions of the whole scene (every decision renders all 64 envs,
    so the scene's own away-from-home assertions hold for each): P0 the scene's
    poses at its times, P1 the same poses at shifted times (the same pose shows
    other objects), P2 the scene turned by one env, poses and times alike.
    fresh: a few envs refill the ring in the middle decision, one in the last."""
    sc = case.scene
    P0 = np.stack([sc.x, sc.z, sc.a])
    T0 = case.t
    T1 = (T0 + np.uint32(case.shift)).astype(np.uint32)
    P2, T2 = np.roll(P0, 1, axis=1), np.roll(case.scene.t, 1)
    poses = [torch.from_numpy(np.ascontiguousarray(p)).to(gpu) for p in (P0, P0, P2)]
    fresh = [torch.zeros(NF, dtype=torch.uint8, device=gpu) for _ in range(3)]
    fresh[1][[0, 3, 17, 40, 63]] = 1
    fresh[2][[3, 5]] = 1
    return poses, [T0, T1, T2], fresh


@pytest.mark.parametrize('frames', ['gray', 'index'])
@pytest.mark.parametrize('k', [2, 3])
def test_grouped_render_with_injected_times(gpu, case, k, frames):
    from aido1_amd.render import RenderOutput, render_group_into
    env = case.env
    poses, times, fresh = injected(case, gpu)
    # expected: k single renders, the handle's counters set before each
    want = RenderOutput(NF, gpu, slots=3, frames=frames)
    env.set_state(step_count=case.other)
    env.render_into(want, pose=poses[0])             # a first frame: the ring is started
    want_masks = []
    for i in range(k):
        env.set_state(step_count=times[i])
        env.render_into(want, fresh=fresh[i], pose=poses[i])
        want_masks.append(want.masks.clone())
    # tested: one launch, the handle's counters elsewhere
    env.set_state(step_count=case.other)
    dts = [case.dev_time(gpu, t) for t in times]
    results = []
    for tt in (dts[:k], [dts[0]] * k):
        got = RenderOutput(NF, gpu, slots=3, frames=frames)
        env.render_into(got, pose=poses[0])
        extra = [torch.full_like(got.masks, 7) for _ in range(k - 1)]
        render_group_into(env, got, extra, fresh[:k], poses[:k], time=tt)
        torch.cuda.synchronize()
        results.append((got, [got.masks] + extra))
    got, got_masks = results[0]
    assert got.slot == want.slot
    assert torch.equal(got.ring, want.ring)
    for i in range(k):
        assert torch.equal(got_masks[i], want_masks[i]), i
    # not vacuous: the same group at [T0, T0, T0] shows other frames
    flat, flat_masks = results[1]
    differs = (flat.ring != want.ring).flatten(1).any(1)
    assert differs.any() and not torch.equal(flat_masks[1], want_masks[1])
    assert np.array_equal(env.get_state()['step_count'], case.other)


# ---- 5: the chunk form end to end ---------------------------------------------------------
@pytest.mark.parametrize('kind', ['walkers', 'bots'])
def test_chunk_then_grouped_renders(gpu, maps, kind):
    """step_many_into(pose=, time=) and two groups of three, against the twin's
    six rounds of step_into + render_into(fresh=done): the final ring and every
    decision's masks.  A respawned env's frame shows the objects at home: the
    twin renders it at step_count 0, the group at time 0."""
    from aido1_amd.render import RenderOutput, render_group_into
    from aido1_amd.vec_env import StepOutput
    n, k = 64, 6
    rng = np.random.default_rng(41)
    env, twin, t0 = start_pair(maps, kind, n, rng, draw=True)
    acts = torch.from_numpy(rng.uniform(0.3, 1.0, (k, n, 2)).astype(F)).to(gpu)
    want = RenderOutput(n, gpu, slots=3, frames='index')
    want_masks, prev, respawns = [], t0, 0
    for d in range(k):
        o = twin.step_into(acts[d])
        twin.render_into(want, fresh=o.done)
        torch.cuda.synchronize()
        want_masks.append(want.masks.clone())
        t = twin.get_state()['step_count']
        respawns += int(((o.done.cpu().numpy() != 0) & (t == 0) & (prev != 0)).sum())
        prev = t
    assert respawns > 0
    out = StepOutput(k * n, gpu, lanepos=False, tile=False)
    pose = torch.zeros(k, 3, n, dtype=torch.float64, device=gpu)
    time = torch.zeros(k, n, dtype=torch.int32, device=gpu)
    env.step_many_into(acts, out, pose=pose, time=time)
    done = out.done.view(k, n)
    got = RenderOutput(n, gpu, slots=3, frames='index')
    got_masks = []
    for d0 in (0, 3):
        extra = [torch.zeros_like(got.masks) for _ in range(2)]
        render_group_into(env, got, extra, [done[d0 + i] for i in range(3)],
                          [pose[d0 + i] for i in range(3)],
                          time=[time[d0 + i] for i in range(3)])
        torch.cuda.synchronize()
        got_masks += [got.masks.clone()] + extra
    assert got.slot == want.slot and torch.equal(got.ring, want.ring)
    for d in range(k):
        assert torch.equal(got_masks[d], want_masks[d]), d
    assert env.check() == 0 and twin.check() == 0


# ---- 6: refusals --------------------------------------------------------------------------
def _err(env):
    return env._L.dt_last_error(env._h).decode()


@pytest.mark.parametrize('kind', ['walkers', 'bots'])
def test_refusals(gpu, maps, kind):
    from aido1_amd import render as RD
    from aido1_amd._lib import DtError
    n = 8
    env = make_env(maps, kind, n, draw=True)
    env.reset()
    L, h = env._L, env._h
    out = RD.RenderOutput(n, gpu, slots=3)
    pose = [torch.zeros(3, n, dtype=torch.float64, device=gpu) for _ in range(3)]
    fresh = [torch.zeros(n, dtype=torch.uint8, device=gpu) for _ in range(3)]
    time = [torch.zeros(n, dtype=torch.int32, device=gpu) for _ in range(3)]
    extra = [torch.zeros_like(out.masks) for _ in range(2)]
    ios = RD._group_ios(env, out, extra, fresh, pose)
    io_arr, t_arr, _ = RD._group_args(ios, time)
    st = env._stream()
    # a dynamic handle: every decision's time, or none of the group
    assert L.dt_render_group(h, io_arr, None, 2, st) == -1
    assert 'dt_render_group' in _err(env) and 'time is required' in _err(env), _err(env)
    for hole in (0, 1):
        holed = (ctypes.c_void_p * 2)(*[None if i == hole else time[i].data_ptr()
                                        for i in range(2)])
        assert L.dt_render_group(h, io_arr, holed, 2, st) == -1
        assert 'dt_render_group' in _err(env) and 'time is required' in _err(env), _err(env)
    holed = (ctypes.c_void_p * 3)(time[0].data_ptr(), time[1].data_ptr(), None)
    assert L.dt_render_group(h, io_arr, holed, 3, st) == -1
    for parts in (0, 4, -1):
        assert L.dt_render_group(h, io_arr, t_arr, parts, st) == -1
        assert 'dt_render_group' in _err(env), _err(env)
    assert L.dt_render_group(h, None, t_arr, 2, st) == -1
    holed = (ctypes.c_void_p * 2)(ctypes.addressof(ios[0]), None)
    assert L.dt_render_group(h, holed, t_arr, 2, st) == -1
    assert 'dt_render_group' in _err(env), _err(env)
    assert L.dt_copy_time(h, None, st) == -1
    # the host API's checks (nothing is launched, the ring does not advance)
    out = RD.RenderOutput(n, gpu, slots=3)
    dev = dict(device=gpu)
    for bad in ([torch.zeros(n, **dev)] + time[1:],
                time[:2] + [torch.zeros(n + 1, dtype=torch.int32, **dev)],
                time[:2], time + time[:1],
                [time[0], torch.zeros(n, 2, dtype=torch.int32, **dev)[:, 0], time[2]],
                time[:2] + [torch.zeros(n, dtype=torch.int32)]):
        with pytest.raises(ValueError, match='time'):
            RD.render_group_into(env, out, extra, fresh, pose, time=bad)
        with pytest.raises(ValueError, match='time'):
            RD.bind_render_group(env, out, torch.cuda.current_stream(gpu), extra, fresh, pose,
                                 time=bad)
    with pytest.raises(ValueError, match='time'):
        RD.render_into(env, out, pose=pose[0], time=torch.zeros(n, **dev))
    assert out.slot == -1
    # without time the existing calls refuse, as before
    with pytest.raises(DtError, match='render walkers or bots'):
        RD.render_group_into(env, RD.RenderOutput(n, gpu, slots=3), extra, fresh, pose)
    # the refusals changed nothing: a valid grouped call renders
    env.copy_pose(pose[0], time=time[0])
    for p, t in zip(pose[1:], time[1:]):
        p.copy_(pose[0])
        t.copy_(time[0])
    single = RD.RenderOutput(n, gpu, slots=3)
    RD.render_into(env, single, pose=pose[0])
    RD.render_group_into(env, out, extra, fresh, pose, time=time)
    assert RD.bind_render_group(env, out, torch.cuda.current_stream(gpu), extra, fresh, pose,
                                time=time)() == 0
    torch.cuda.synchronize()
    assert torch.equal(out.masks, single.masks) and torch.equal(extra[1], single.masks)
    assert torch.equal(out.ring, single.ring)      # every slot holds the one frame
    assert env.check() == 0


def test_static_handle_ignores_time(gpu, maps):
    """Static objects drawn, no walkers or bots: time given or not, one output."""
    from aido1_amd.render import RenderOutput, render_group_into
    n = 8
    env = make_env(maps, 'static', n, draw=True)
    assert not env.map.has_walkers
    env.reset()
    pose = [torch.zeros(3, n, dtype=torch.float64, device=gpu) for _ in range(3)]
    env.copy_pose(pose[0])
    env.step_into(torch.full((n, 2), 0.6, device=gpu))
    env.copy_pose(pose[1])
    env.step_into(torch.full((n, 2), 0.6, device=gpu))
    env.copy_pose(pose[2])
    fresh = [torch.zeros(n, dtype=torch.uint8, device=gpu) for _ in range(3)]
    time = [torch.full((n,), 50 * (i + 1), dtype=torch.int32, device=gpu) for i in range(3)]
    res = []
    for tt in (None, time):
        out = RenderOutput(n, gpu, slots=3)
        extra = [torch.zeros_like(out.masks) for _ in range(2)]
        render_group_into(env, out, extra, fresh, pose, time=tt)
        one = RenderOutput(n, gpu, slots=1, rgb=True)
        env.render_into(one, pose=pose[1], time=None if tt is None else tt[1])
        torch.cuda.synchronize()
        res.append([out.ring, out.masks] + extra + [one.rgb, one.masks, one.ring])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert env.check() == 0
