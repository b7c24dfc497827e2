"""GPU: the forward-camera observation (VecEnv(camera=...), dt_render_camera,
render_kernel's phase 0d).  The expected frame is always a numpy gather
(tests/ego_ref.py) of a top-down frame through the table: the twin handle's,
or oracle/render_oracle.c's, with the oracle's line detector on the gathered
image.  Everything is compared bit for bit: rgb, the grey and index rings, the
masks."""
import ctypes

import numpy as np
import pytest
import torch

import ego_ref as ER
import render_objects_ref as RO
from conftest import golden, map_rows
from oracle import oracle_c as OC

pytestmark = pytest.mark.gpu

N = 64
SEED = 3
NONE = 0xFFFF


def make_env(map_name='loop_empty', camera=None, seed=SEED, n=N, **kw):
    from aido1_amd.config import EnvConfig
    from aido1_amd.vec_env import VecEnv
    env = VecEnv(n, seed=seed, config=EnvConfig(map_name=map_name), camera=camera, **kw)
    env.reset()
    return env


def synthetic_tables():
    ident = np.arange(19200, dtype=np.uint16).reshape(120, 160)
    rng = np.random.default_rng(11)
    rnd = rng.integers(0, 19200, 19200).astype(np.uint16)
    rnd[rng.random(19200) < 0.2] = NONE
    rnd[5], rnd[6] = 0, 19199
    return {'identity': ident, 'reversed': (19199 - ident).astype(np.uint16),
            'random': rnd.reshape(120, 160)}


class Scene:
    """loop_empty, seed 3: the 64 reset poses and the twin handle's top-down
    outputs at them (rgb, grey frame, index frame), rendered once."""

    def __init__(self, dev):
        from aido1_amd.render import RenderOutput
        env = make_env()
        s = env.get_state()
        self.x, self.z, self.a = s['x'], s['z'], s['angle']
        self.top = {}
        for frames in ('gray', 'index'):
            out = RenderOutput(N, dev, slots=1, rgb=True, frames=frames)
            env.render_into(out, pose=self.pose(dev))
            torch.cuda.synchronize()
            self.top[frames] = out.ring[:, 0].cpu().numpy()
            self.rgb = out.rgb.cpu().numpy()
            self.masks = out.masks.cpu().numpy()
        env.close()
        self.orend = OC.OracleRender(map_rows('loop_empty'))
        # the twin is the oracle's frame (tests/test_gpu_render.py pins that; here it keeps
        # the two references of this file one)
        _, _, rgb = self.orend.render(self.x, self.z, self.a)
        assert np.array_equal(rgb, self.rgb)

    def pose(self, dev, shift=0):
        p = np.stack([np.roll(v, shift) for v in (self.x, self.z, self.a)])
        return torch.from_numpy(np.ascontiguousarray(p)).to(dev)

    def expect(self, table, frames, orend=None):
        """(ring frame, masks, rgb) of the forward view through `table`."""
        rgb = ER.gather(self.rgb, table)
        masks = (orend or self.orend).line_detect(rgb[..., ::-1])
        return ER.gather(self.top[frames], table), masks, rgb


@pytest.fixture(scope='module')
def scene(gpu):
    return Scene(gpu)


def check(out, want):
    torch.cuda.synchronize()
    ring, masks, rgb = want
    assert np.array_equal(out.rgb.cpu().numpy(), rgb)
    assert np.array_equal(out.ring[:, 0].cpu().numpy(), ring)
    assert np.array_equal(out.masks.cpu().numpy(), masks)


@pytest.mark.parametrize('list_cap', [0, 64], ids=['lds', 'spill'])
@pytest.mark.parametrize('frames', ['gray', 'index'])
def test_synthetic_tables_through_the_abi(gpu, scene, frames, list_cap):
    """Identity, reversed and random tables (about 20 % 0xFFFF; entries 0 and
    19199 present), uploaded one after the other into one handle; list_cap 64
    puts the listed words of every such frame past the LDS list.  Then the
    all-0xFFFF table: a black frame, empty masks, no fault."""
    from aido1_amd.render import RenderOutput
    env = make_env()
    out = RenderOutput(N, gpu, slots=1, rgb=True, frames=frames)
    tabs = synthetic_tables()
    assert 0 in tabs['random'] and 19199 in tabs['random']
    assert 0.15 < (tabs['random'] == NONE).mean() < 0.25
    for name, t in tabs.items():
        env.set_camera(t)
        env.render_into(out, pose=scene.pose(gpu), list_cap=list_cap)
        want = scene.expect(t, frames)
        check(out, want)
        assert (want[1][:, 3] > 0).any() and (want[1][:, 0] > 0).any(), name
        if name == 'identity':   # ... is the top-down output itself
            assert np.array_equal(want[2], scene.rgb) and np.array_equal(want[1], scene.masks)
    env.set_camera(np.full((120, 160), NONE, np.uint16))
    env.render_into(out, pose=scene.pose(gpu), list_cap=list_cap)
    torch.cuda.synchronize()
    assert not out.rgb.any() and not out.masks.any() and not out.ring.any()
    assert env.check() == 0


@pytest.mark.parametrize('distortion', [False, True], ids=['pinhole', 'distorted'])
@pytest.mark.parametrize('map_name', ['loop_empty', 'intersections'])
def test_default_camera_matches_gathered_oracle(gpu, map_name, distortion):
    """camera='ego' / EgoCamera(distortion=True) against the gathered
    OracleRender.render frame and the oracle's line detector on it, with the
    default 3 x 3 dilation and with size 5 (the radius-2 output path)."""
    from aido1_amd.camera import EgoCamera
    from aido1_amd.render import LineParams, RenderOutput
    cam = EgoCamera(distortion=True) if distortion else 'ego'
    env = make_env(map_name, camera=cam)
    assert env.camera.distortion == distortion
    table = EgoCamera(distortion=distortion).table()
    s = env.get_state()
    rows = map_rows(map_name)
    gray, _, rgb = OC.OracleRender(rows).render(s['x'], s['z'], s['angle'])
    fwd = ER.gather(rgb, table)
    assert not np.array_equal(fwd, rgb)
    for size in (3, 5):
        op = OC.line_params_default()
        op.dilation_kernel_size = size
        masks = OC.OracleRender(rows, params=op).line_detect(fwd[..., ::-1])
        p = LineParams.default()
        p.dilation_kernel_size = size
        env.set_line_params(p)
        out = RenderOutput(N, gpu, slots=1, rgb=True)
        env.render_into(out)
        check(out, (ER.gather(gray, table), masks, fwd))
        assert (masks[:, 3] > 0).any((1, 2)).mean() > 0.9


@pytest.mark.parametrize('frames', ['gray', 'index'])
@pytest.mark.parametrize('k', [2, 3])
def test_grouped_launches_match_single_renders(gpu, scene, frames, k):
    """dt_render2 / dt_render3 (and, with times given, dt_render_group) on a
    handle with the camera on equal k single renders in order: fresh flags set
    in some envs, four groups; the last decision's frame is the gather."""
    from aido1_amd.camera import EgoCamera
    from aido1_amd.render import RenderOutput, render_group_into
    env = make_env(camera='ego')
    table = EgoCamera().table()
    ref = RenderOutput(N, gpu, frames=frames)
    grp = RenderOutput(N, gpu, frames=frames)
    extra = [torch.zeros_like(grp.masks) for _ in range(k - 1)]
    g = torch.Generator(device=gpu)
    g.manual_seed(7)
    zero = torch.zeros(N, dtype=torch.int32, device=gpu)
    for it in range(4):
        poses = [scene.pose(gpu, shift=k * it + d) for d in range(k)]
        fresh = [(torch.rand(N, generator=g, device=gpu) < 0.3).to(torch.uint8) for _ in range(k)]
        want = []
        for f, p in zip(fresh, poses):
            env.render_into(ref, fresh=f, pose=p)
            want.append(ref.masks.clone())
        render_group_into(env, grp, extra, fresh, poses, time=[zero] * k if it & 1 else None)
        torch.cuda.synchronize()
        assert grp.slot == ref.slot
        for got, w in zip([grp.masks] + extra, want):
            assert torch.equal(got, w), it
            assert (got[:, 3] > 0).any()
        assert torch.equal(grp.ring, ref.ring), it
    last = np.roll(ER.gather(scene.top[frames], table), k * 3 + k - 1, axis=0)
    assert np.array_equal(grp.ring[:, grp.slot].cpu().numpy(), last)


def mover_poses(centres, rng):
    """N poses, pose i with the point centres[i] 0.2 .. 0.6 m ahead of the
    camera and within 0.1 m of its axis: inside the forward view."""
    x, z, a = np.zeros(N), np.zeros(N), np.zeros(N)
    for i in range(N):
        a[i] = rng.uniform(-np.pi, np.pi)
        x[i], z[i] = RO.pose_seeing(centres[i][0], centres[i][1], a[i], rng.uniform(0.2, 0.6),
                                    rng.uniform(-0.1, 0.1))
    return x, z, a


@pytest.mark.parametrize('map_name', ['loop_pedestrians', 'loop_dyn_duckiebots'])
def test_movers_come_through_the_camera(gpu, map_name):
    """draw_objects=True with walkers (time= given) and with lane-following
    bots: the forward frame is the gather of a twin's top-down frame at the
    same pose and time, and the movers are in it."""
    from aido1_amd.camera import EgoCamera
    from aido1_amd.render import RenderOutput
    bots = map_name == 'loop_dyn_duckiebots'
    kw = dict(draw_objects=True, lane_bots=bots, bot_rows=512 if bots else None)
    twin = make_env(map_name, **kw)
    env = make_env(map_name, camera=EgoCamera(distortion=True), **kw)
    table = env.camera.table()
    rng = np.random.default_rng(5)
    t = rng.integers(0, 500, N).astype(np.uint32)
    if bots:
        centres = [twin.bot_path[t[i], i % 3, :2] for i in range(N)]
    else:
        from aido1_amd.maps import walker_index
        walkers = [o for o in twin.map.objects if o.walker]
        assert walkers
        centres = []
        for i in range(N):     # where walker i % len stands at time t[i]
            o = walkers[i % len(walkers)]
            k = walker_index(t[i], o.W, o.K) * o.vel
            centres.append(o.corners.mean(0) + k * np.array(o.heading))
    x, z, a = mover_poses(centres, rng)
    pose = torch.from_numpy(np.ascontiguousarray(np.stack([x, z, a]))).to(gpu)
    time = torch.from_numpy(t.view(np.int32)).to(gpu)
    red = np.array(RO.RED, np.uint8)
    for frames in ('gray', 'index'):
        outs = [RenderOutput(N, gpu, slots=1, rgb=True, frames=frames) for _ in range(2)]
        twin.render_into(outs[0], pose=pose, time=time)
        env.render_into(outs[1], pose=pose, time=time)
        torch.cuda.synchronize()
        rgb = ER.gather(outs[0].rgb.cpu().numpy(), table)
        masks = OC.OracleRender(map_rows(map_name)).line_detect(rgb[..., ::-1])
        check(outs[1], (ER.gather(outs[0].ring[:, 0].cpu().numpy(), table), masks, rgb))
        seen = (rgb == red).all(-1).any((1, 2))
        assert seen.mean() >= 0.5, seen.mean()
        assert (masks[:, 2] > 0).any()
    # another time is another frame: the movers moved
    twin.render_into(outs[0], pose=pose, time=time + 40)
    env.render_into(outs[1], pose=pose, time=time + 40)
    torch.cuda.synchronize()
    rgb2 = ER.gather(outs[0].rgb.cpu().numpy(), table)
    assert np.array_equal(outs[1].rgb.cpu().numpy(), rgb2) and not np.array_equal(rgb2, rgb)
    assert env.check() == 0 and twin.check() == 0


def test_switching_off_restores_the_top_down_frame(gpu, scene):
    from aido1_amd.render import RenderOutput
    env = make_env(camera='ego')
    out = RenderOutput(N, gpu, slots=1, rgb=True)
    env.render_into(out, pose=scene.pose(gpu))
    torch.cuda.synchronize()
    assert not np.array_equal(out.rgb.cpu().numpy(), scene.rgb)
    env.set_camera(None)
    assert env.camera is None
    env.render_into(out, pose=scene.pose(gpu))
    check(out, (scene.top['gray'], scene.masks, scene.rgb))


def test_a_bad_table_is_refused(gpu, scene):
    """An entry of 19200 (and 65534, a wrong count, a null table with a count):
    a non-zero status with a message, and the next render is unchanged."""
    from aido1_amd.camera import EgoCamera
    from aido1_amd.render import RenderOutput
    env = make_env(camera='ego')
    good = EgoCamera().table()
    want = scene.expect(good, 'gray')
    L, h = env._L, env._h
    for v in (19200, 65534):
        bad = np.ascontiguousarray(good[::-1])    # another table, were it accepted
        bad[60, 80] = v
        assert L.dt_render_camera(h, bad.ctypes.data_as(ctypes.c_void_p), 19200) == -1
        assert b'dt_render_camera' in L.dt_last_error(h)
        with pytest.raises(ValueError):
            env.set_camera(bad)
    p = good.ctypes.data_as(ctypes.c_void_p)
    for n in (19199, 19201, 0, -1):
        assert L.dt_render_camera(h, p, n) == -1
    assert L.dt_render_camera(h, None, 19200) == -1
    assert L.dt_render_camera(None, p, 19200) == -1
    out = RenderOutput(N, gpu, slots=1, rgb=True)
    env.render_into(out, pose=scene.pose(gpu))
    check(out, want)


def test_captured_render_follows_a_replaced_table(gpu, scene):
    """A render captured into a graph with the camera on reads the handle's
    one table allocation: after set_camera with another table the replay
    draws through the new one."""
    from aido1_amd.camera import EgoCamera
    from aido1_amd.render import RenderOutput
    env = make_env(camera='ego')
    out = RenderOutput(N, gpu, slots=1, rgb=True, frames='index')
    pose = scene.pose(gpu)
    env.render_into(out, pose=pose)     # (the first render of a ring fills every slot: not captured)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.render_into(out, pose=pose)
    for cam in (EgoCamera(distortion=True), EgoCamera(0.12, 25.0, 60.0), EgoCamera()):
        env.set_camera(cam)
        out.rgb.zero_()
        out.masks.zero_()
        out.ring.zero_()
        graph.replay()
        check(out, scene.expect(cam.table(), 'index'))


def test_simulator_and_rollout_take_the_camera(gpu):
    """Simulator(camera='ego', distortion=True) observes what the batched path
    renders at its pose; without camera= distortion stays ignored; and
    ActorRollout(camera='ego') acts on index frames."""
    from aido1_amd.camera import EgoCamera
    from aido1_amd.env_server import GpuBatch
    from aido1_amd.render import RenderOutput
    from aido1_amd.rollout import ActorRollout
    from aido1_amd.simulator import Simulator
    sim = Simulator(seed=SEED, device=0, camera='ego', distortion=True)
    assert sim._env.camera.distortion
    obs = [sim.reset(), sim.step(np.array([0.6, 0.4]))[0]]
    assert obs[1].shape == (120, 160, 3)
    s = sim._env.get_state()
    env = make_env(camera=EgoCamera(distortion=True), n=1)
    env.set_state(x=s['x'], z=s['z'], angle=s['angle'])
    out = RenderOutput(1, gpu, slots=1, rgb=True, masks=False)
    env.render_into(out)
    torch.cuda.synchronize()
    assert np.array_equal(out.rgb[0].cpu().numpy(), obs[1])
    rgb = OC.OracleRender(map_rows('loop_empty')).render(s['x'], s['z'], s['angle'])[2]
    assert np.array_equal(ER.gather(rgb, EgoCamera(distortion=True).table())[0], obs[1])
    assert not obs[1][:40].any() and obs[1][60:].any()      # sky above the horizon
    plain = Simulator(seed=SEED, device=0, distortion=True)
    assert plain._env.camera is None
    assert not np.array_equal(plain.reset(), obs[0]) and plain.reset()[:40].any()
    batch = GpuBatch(2, device=0, camera='ego')
    assert not batch.env.camera.distortion
    torch.manual_seed(1)
    roll = ActorRollout(golden('reference_config.json'), N, maps=('loop_empty',), device=0,
                        seed=21, frames='index', camera='ego')
    roll.reset()
    for _ in range(3):
        roll.step()
    torch.cuda.synchronize()
    assert torch.isfinite(roll.actions).all()
    newest = roll.ring[:, roll.renders[0].slot]
    assert newest.dtype == torch.uint8
    s = roll.envs[0].get_state()
    top = OC.OracleRender(map_rows('loop_empty')).render(s['x'], s['z'], s['angle'])[0]
    from aido1_amd.render import decode_index
    assert np.array_equal(decode_index(newest).cpu().numpy(), ER.gather(top, EgoCamera().table()))
    assert roll.envs[0].check() == 0
    roll.close()
