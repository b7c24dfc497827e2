"""GPU: the map's objects drawn into the observation (VecEnv(draw_objects=True),
dt_render_objects) against the composed oracle of tests/render_objects_ref.py:
oracle/render_oracle.c's object-free frame, the footprints painted red by the
float32 restatement, the oracle's line detector on that image.  Every output
is compared bit for bit."""
import ctypes
import math

import numpy as np
import pytest
import torch

import render_objects_ref as RO
from conftest import golden, map_objects, map_rows
from oracle import oracle_c as OC

pytestmark = pytest.mark.gpu

MAP = 'loop_obstacles'
N = 64


class Scene:
    """64 poses around loop_obstacles' objects and their expected frames."""

    def __init__(self):
        from aido1_amd.maps import load_map
        m = load_map(MAP)
        self.table = m.render_table
        centres = [o.corners.mean(0) for o in m.objects]
        x, z, a = RO.place_poses(centres, np.random.default_rng(3), N - 10)
        edge = []   # the tree and the house across the bottom, top, left and right edge
        for k, turn in ((3, 0.4), (4, -2.0)):
            for ahead, lat in ((0.0, 0.1), (1.2, -0.2), (0.5, -0.8), (0.7, 0.8)):
                edge.append(RO.pose_seeing(*centres[k], turn, ahead, lat) + (turn,))
                turn += 0.9
        # nothing in view: far off the map; on it, looking away from every object
        none = [(-40.0, 7.0, 1.0), (0.3, 0.3, 0.75 * math.pi)]
        extra = np.array(edge + none)
        self.x, self.z, self.a = (np.r_[v, extra[:, i]] for i, v in enumerate((x, z, a)))
        self.orend = OC.OracleRender(map_rows(MAP))
        self.gray, self.masks, self.rgb, self.obj = RO.compose(self.orend, self.table, self.x,
                                                               self.z, self.a)
        per = self.obj.reshape(N, -1).sum(1)
        # not vacuous: objects in most frames, across every edge, and the two empty frames
        assert (per > 0).mean() >= 0.8, per
        assert (per[-2:] == 0).all()
        o = self.obj[N - 10:N - 2]
        for k in (0, 4):
            assert o[k, -1].any() and o[k + 1, 0].any() and o[k + 2, :, 0].any() and \
                o[k + 3, :, -1].any(), k
        assert (self.masks[:, 2][self.obj] == 255).all()    # the red mask covers the objects
        assert (self.masks[:, 3] > 0).any()

    def pose(self, dev, shift=0):
        p = np.stack([np.roll(v, shift) for v in (self.x, self.z, self.a)])
        return torch.from_numpy(np.ascontiguousarray(p)).to(dev)


@pytest.fixture(scope='module')
def scene():
    return Scene()


def make_env(map_name=MAP, draw=True, seed=3):
    from aido1_amd.config import EnvConfig
    from aido1_amd.vec_env import VecEnv
    env = VecEnv(N, seed=seed, config=EnvConfig(map_name=map_name), draw_objects=draw)
    env.reset()
    return env


def check_frame(out, want_gray, want_masks, want_rgb, obj):
    from aido1_amd.render import decode_index
    torch.cuda.synchronize()
    assert np.array_equal(out.rgb.cpu().numpy(), want_rgb)
    assert np.array_equal(out.masks.cpu().numpy(), want_masks)
    ring = out.ring[:, 0]
    if ring.dtype == torch.uint8:
        assert np.array_equal(ring.cpu().numpy() == RO.PAL_RED, obj)
        ring = decode_index(ring)
    assert np.array_equal(ring.cpu().numpy(), want_gray)


@pytest.mark.parametrize('list_cap', [0, 64], ids=['lds', 'spill'])
@pytest.mark.parametrize('frames', ['gray', 'index'])
def test_objects_match_composed_oracle(gpu, scene, frames, list_cap):
    """rgb, masks and the grey / index ring; list_cap 64 forces the listed
    words of nearly every frame here past the LDS list."""
    from aido1_amd.render import RenderOutput
    env = make_env()
    out = RenderOutput(N, gpu, slots=1, rgb=True, frames=frames)
    env.render_into(out, pose=scene.pose(gpu), list_cap=list_cap)
    check_frame(out, scene.gray, scene.masks, scene.rgb, scene.obj)


@pytest.mark.parametrize('frames', ['gray', 'index'])
def test_objects_with_dilation_5(gpu, scene, frames):
    """dilation_kernel_size 5: the radius-2 output path, against the oracle's
    line detector with the same parameters."""
    from aido1_amd.render import LineParams, RenderOutput
    op = OC.line_params_default()
    op.dilation_kernel_size = 5
    masks = OC.OracleRender(map_rows(MAP), params=op).line_detect(scene.rgb[..., ::-1])
    assert not np.array_equal(masks, scene.masks)
    env = make_env()
    p = LineParams.default()
    p.dilation_kernel_size = 5
    env.set_line_params(p)
    out = RenderOutput(N, gpu, slots=1, rgb=True, frames=frames)
    env.render_into(out, pose=scene.pose(gpu))
    check_frame(out, scene.gray, masks, scene.rgb, scene.obj)


@pytest.mark.parametrize('frames', ['gray', 'index'])
@pytest.mark.parametrize('k', [2, 3])
def test_render_group_matches_single_renders(gpu, scene, frames, k):
    """dt_render2 / dt_render3 on an env that draws objects equal k single
    renders in order: the ring and every decision's masks, fresh flags set in
    some envs, over several groups (the form of
    test_render3_matches_three_renders)."""
    from aido1_amd.render import RenderOutput, render_group_into
    env = make_env()
    ref = RenderOutput(N, gpu, frames=frames)
    grp = RenderOutput(N, gpu, frames=frames)
    extra = [torch.zeros_like(grp.masks) for _ in range(k - 1)]
    g = torch.Generator(device=gpu)
    g.manual_seed(7)
    for it in range(4):
        poses = [scene.pose(gpu, shift=k * it + d) for d in range(k)]
        fresh = [(torch.rand(N, generator=g, device=gpu) < 0.3).to(torch.uint8) for _ in range(k)]
        want = []
        for f, p in zip(fresh, poses):
            env.render_into(ref, fresh=f, pose=p)
            want.append(ref.masks.clone())
        render_group_into(env, grp, extra, fresh, poses)
        torch.cuda.synchronize()
        assert grp.slot == ref.slot
        for got, w in zip([grp.masks] + extra, want):
            assert torch.equal(got, w), it
            assert (got[:, 2] > 0).any()
        assert torch.equal(grp.ring, ref.ring), it
    # the last decision's frame is the composed oracle's at its poses
    last = np.roll(scene.gray, k * 3 + k - 1, axis=0)
    from aido1_amd.render import as_gray
    assert np.array_equal(as_gray(grp.ring[:, grp.slot]).cpu().numpy(), last)


@pytest.mark.parametrize('map_name,draw', [(MAP, False), ('loop_empty', True)])
def test_off_means_off(gpu, scene, map_name, draw):
    """Without the switch, or on a map without objects, the frame is the plain
    oracle's, as it has always been."""
    from aido1_amd.render import RenderOutput
    env = make_env(map_name, draw)
    out = RenderOutput(N, gpu, slots=1, rgb=True)
    env.render_into(out, pose=scene.pose(gpu))
    torch.cuda.synchronize()
    g, m, rgb = OC.OracleRender(map_rows(map_name)).render(scene.x, scene.z, scene.a)
    assert np.array_equal(out.rgb.cpu().numpy(), rgb)
    assert np.array_equal(out.masks.cpu().numpy(), m)
    assert np.array_equal(out.ring[:, 0].cpu().numpy(), g)
    assert not (m[:, 2] > 0).any()


def test_step_graph_with_render_replays_like_eager(gpu, scene):
    """Steps and renders of an env that draws objects, captured into a HIP
    graph: two replays leave the ring and the masks as the eager launches do."""
    from aido1_amd.render import RenderOutput
    envs = [make_env(seed=9) for _ in range(2)]
    outs = [RenderOutput(N, gpu, frames='index') for _ in range(2)]
    for env, ro in zip(envs, outs):
        env.set_state(x=scene.x, z=scene.z, angle=scene.a)
        env.render_into(ro)
    rng = np.random.default_rng(5)
    acts = torch.from_numpy(rng.uniform(0, 1, (6, N, 2)).astype(np.float32)).to(gpu)
    buf = torch.empty(3, N, 2, dtype=torch.float32, device=gpu)
    sg = envs[1].capture(buf, render=outs[1])
    for c in range(2):
        for k in range(3):
            o = envs[0].step_into(acts[3 * c + k])
            envs[0].render_into(outs[0], fresh=o.done)
        buf.copy_(acts[3 * c:3 * c + 3])
        sg.replay()
        torch.cuda.synchronize()
        assert outs[0].slot == outs[1].slot
        assert torch.equal(outs[0].ring, outs[1].ring), c
        assert torch.equal(outs[0].masks, outs[1].masks), c
    assert (outs[1].ring == RO.PAL_RED).any() and (outs[1].masks[:, 2] > 0).any()
    for env in envs:
        env.check()


def test_render_objects_refuses_bad_arguments(gpu, scene):
    """n < 0, n > 256, null records with n > 0 and a non-finite value: DT_E_ARG
    with a message, and the handle keeps drawing what it drew."""
    from aido1_amd.render import RenderOutput
    env = make_env()
    L, h = env._L, env._h
    big = np.zeros((257, 8), np.float32)
    bad = [(scene.table, -1), (big, 257), (None, 1)]
    for v in (np.nan, np.inf, -np.inf):
        t = scene.table.copy()
        t[2, 5] = v
        bad.append((t, len(t)))
    for t, n in bad:
        p = t.ctypes.data_as(ctypes.c_void_p) if t is not None else None
        assert L.dt_render_objects(h, p, n) == -1
        assert b'dt_render_objects' in L.dt_last_error(h)
    assert L.dt_render_objects(None, None, 0) == -1
    out = RenderOutput(N, gpu, slots=1, rgb=True)
    env.render_into(out, pose=scene.pose(gpu))
    check_frame(out, scene.gray, scene.masks, scene.rgb, scene.obj)
    # n = 0 switches the drawing off again
    assert L.dt_render_objects(h, None, 0) == 0
    env.render_into(out, pose=scene.pose(gpu))
    torch.cuda.synchronize()
    assert not (out.masks[:, 2] > 0).any()
    assert not (out.rgb.cpu().numpy() == RO.RED).all(-1).any()


def test_rollout_sees_the_objects(gpu, scene):
    """ActorRollout(frames='index', draw_objects=True) on loop_obstacles: after
    a few decisions the newest ring slot is the restatement at the poses read
    back, and objects are in it.  Seed 21 spawns 55 of the 64 envs with an
    object in view (the CPU oracle's reset, checked first)."""
    from aido1_amd.rollout import ActorRollout
    seed = 21
    ob = OC.OracleBatch(map_rows(MAP), N, seed=seed, objects=map_objects(MAP))
    ob.reset()
    s0 = ob.state()
    assert RO.object_mask(scene.table, s0['x'], s0['z'], s0['angle']).any((1, 2)).sum() >= 32
    torch.manual_seed(1)
    roll = ActorRollout(golden('reference_config.json'), N, maps=(MAP,), device=0, seed=seed,
                        frames='index', draw_objects=True)
    roll.reset()
    for _ in range(3):
        roll.step()
    torch.cuda.synchronize()
    s = roll.envs[0].get_state()
    gray, _, _, obj = RO.compose(scene.orend, scene.table, s['x'], s['z'], s['angle'])
    newest = roll.ring[:, roll.renders[0].slot]
    assert newest.dtype == torch.uint8
    assert obj.any() and np.array_equal(newest.cpu().numpy() == RO.PAL_RED, obj)
    from aido1_amd.render import decode_index
    assert np.array_equal(decode_index(newest).cpu().numpy(), gray)
    assert roll.envs[0].check() == 0
    roll.close()
