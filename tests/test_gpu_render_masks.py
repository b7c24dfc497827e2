"""The render kernel's mask path with a dilation radius <= 1: Canny's NMS
dilates the colour bits of the listed words (words whose 3 x 6-pixel
neighbourhood is not one colour) and parks them in the work entries beside the
candidate / edge flags; the output phase only unpacks them.  Grey and all four
masks against the C oracle (oracle/render_oracle.c), bit for bit, where that
hand-over can go wrong: listed words on the image borders (a clipped
neighbourhood), hysteresis rewriting entries that hold parked bits, the
grouped launch, and launches that change streams (the order event)."""
import math

import numpy as np
import pytest
import torch

from conftest import map_rows
from oracle import oracle_c as OC

pytestmark = pytest.mark.gpu

H, W = 120, 160


def _env(map_name, n, seed):
    from aido1_amd.config import EnvConfig
    from aido1_amd.vec_env import VecEnv
    env = VecEnv(n, seed=seed, config=EnvConfig(map_name=map_name))
    env.reset()
    return env


def _jitter(s, rng, shift=0.25, turn=1.0):
    """Spawn poses (on a lane, the markings in view) shifted and rotated by
    seeded amounts: the markings leave the frame through every border."""
    n = len(s['x'])
    return (s['x'] + rng.uniform(-shift, shift, n), s['z'] + rng.uniform(-shift, shift, n),
            s['angle'] + rng.uniform(-turn, turn, n))


def _params(dil, lo, hi):
    from aido1_amd.render import LineParams
    lp, p = LineParams.default(), OC.line_params_default()
    lp.dilation_kernel_size = p.dilation_kernel_size = dil
    lp.canny_lo, lp.canny_hi = p.canny_lo, p.canny_hi = lo, hi
    return lp, p


def _check(out, g, m, slot=0):
    assert np.array_equal(out.masks.cpu().numpy(), m)
    assert np.array_equal(out.ring[:, slot].cpu().numpy(), g)


BORDERS = {'row 0': np.s_[..., 0, :], 'row 119': np.s_[..., H - 1, :],
           'column 0': np.s_[..., :, 0], 'column 159': np.s_[..., :, W - 1]}


@pytest.mark.parametrize('dil', [1, 3])
@pytest.mark.parametrize('map_name', ['loop_empty', 'zigzag'])
def test_listed_words_on_every_border(gpu, map_name, dil):
    """Markings cross rows 0 and 119 and columns 0 and 159: NMS's 3 x 3 word
    neighbourhood of those listed words is clipped (rows and side words
    outside the image give no colour bits)."""
    from aido1_amd.render import RenderOutput
    n = 128
    env = _env(map_name, n, seed=31)
    x, z, a = _jitter(env.get_state(), np.random.default_rng(32))
    env.set_state(x=x, z=z, angle=a)
    lp, p = _params(dil, 80.0, 200.0)
    env.set_line_params(lp)
    out = RenderOutput(n, gpu, slots=1)
    env.render_into(out)
    torch.cuda.synchronize()
    g, m, _ = OC.OracleRender(map_rows(map_name), params=p).render(x, z, a)
    # the case is what it says: a colour mask and an edge on every border
    for name, sl in BORDERS.items():
        assert (m[:, :3][sl] > 0).any() and (m[:, 3][sl] > 0).any(), name
    _check(out, g, m)


# canny_hi 2041 is above any magnitude (the L1 Sobel of 8-bit channels is at
# most 2040): every candidate is weak and none may become an edge
@pytest.mark.parametrize('list_cap', [0, 64])
@pytest.mark.parametrize('hi', [1200.0, 2041.0])
def test_hysteresis_keeps_parked_bits(gpu, hi, list_cap):
    """Most candidates weak (a low canny_lo, a high canny_hi): hysteresis visits
    and rewrites the entries that hold the dilated colour bits.  With the
    default list and with list_cap = 64 (the spill instantiation)."""
    from aido1_amd.render import RenderOutput
    n, lo = 128, 20.0
    env = _env('loop_empty', n, seed=33)
    x, z, a = _jitter(env.get_state(), np.random.default_rng(34), shift=0.1, turn=0.5)
    env.set_state(x=x, z=z, angle=a)
    lp, p = _params(3, lo, hi)
    env.set_line_params(lp)
    out = RenderOutput(n, gpu, slots=1)
    env.render_into(out, list_cap=list_cap)
    torch.cuda.synchronize()
    rows = map_rows('loop_empty')
    g, m, _ = OC.OracleRender(rows, params=p).render(x, z, a)
    if hi > 2040.0:
        assert not m[:, 3].any()
    else:
        # edges propagate: more of them than the strong pixels alone
        _, p_strong = _params(3, hi, hi)
        _, ms, _ = OC.OracleRender(rows, params=p_strong).render(x, z, a)
        strong = int((ms[:, 3] > 0).sum())
        assert strong > 0 and int((m[:, 3] > 0).sum()) > 2 * strong
    assert (m[:, 0] > 0).any() and (m[:, 1] > 0).any()
    _check(out, g, m)


def test_grouped_launch_masks(gpu):
    """One dt_render3 launch at 640 envs (the dispatch order is live), fresh
    flags on some envs in the middle decision: each decision's masks buffer
    and the ring equal three single renders' oracle outputs."""
    from aido1_amd.render import RenderOutput, render_group_into
    n = 640
    env = _env('loop_empty', n, seed=35)
    rng = np.random.default_rng(36)
    s = env.get_state()
    orend = OC.OracleRender(map_rows('loop_empty'))   # dilation size 3, the default
    grp = RenderOutput(n, gpu)
    env.render_into(grp)                 # the ring's first frame: every slot
    extra = [torch.zeros_like(grp.masks) for _ in range(2)]
    pose_np = [_jitter(s, rng) for _ in range(3)]
    poses = [torch.from_numpy(np.stack(p)).to(gpu) for p in pose_np]
    mid = (rng.random(n) < 0.3).astype(np.uint8)
    zero = torch.zeros(n, dtype=torch.uint8, device=gpu)
    fresh = [zero, torch.from_numpy(mid).to(gpu), zero]
    render_group_into(env, grp, extra, fresh, poses)
    torch.cuda.synchronize()
    want = [orend.render(*p) for p in pose_np]
    for got, (_, m, _) in zip([grp.masks] + extra, want):
        assert np.array_equal(got.cpu().numpy(), m)
    ring = grp.ring.cpu().numpy()
    slots = [1, 2, 0]                    # the three decisions' slots after the first frame
    g = [w[0] for w in want]
    f = mid.astype(bool)
    assert grp.slot == 0
    assert np.array_equal(ring[:, slots[2]], g[2])
    assert np.array_equal(ring[:, slots[1]], g[1])
    assert np.array_equal(ring[~f, slots[0]], g[0][~f])
    assert np.array_equal(ring[f, slots[0]], g[1][f])     # the respawn's frame fills the ring


def test_cross_stream_launch_order(gpu):
    """Six dt_render launches of 640 envs alternate between two streams with no
    host synchronisation in between, each after new poses arrive on the
    launching stream; one device synchronise at the end.  The launches share
    the dispatch-order state and the output buffers, so each must wait for the
    one before it on the other stream: the last launch's outputs are the
    oracle's, and the order state saw six launches and holds a permutation.
    (The poses arrive as pose snapshots copied on the launching stream:
    VecEnv.set_state synchronises the device, which would order the launches
    by itself.)"""
    from aido1_amd.render import RenderOutput
    n, k = 640, 6
    env = _env('loop_empty', n, seed=37)
    rng = np.random.default_rng(38)
    s = env.get_state()
    pose_np = [_jitter(s, rng) for _ in range(k)]
    host = [torch.from_numpy(np.stack(p)).pin_memory() for p in pose_np]
    dev = [torch.empty(3, n, dtype=torch.float64, device=gpu) for _ in range(k)]
    out = RenderOutput(n, gpu, slots=1)
    streams = [torch.cuda.Stream(device=gpu) for _ in range(2)]
    torch.cuda.synchronize()
    for i in range(k):
        with torch.cuda.stream(streams[i & 1]):
            dev[i].copy_(host[i], non_blocking=True)
            env.render_into(out, pose=dev[i])
    torch.cuda.synchronize()
    g, m, _ = OC.OracleRender(map_rows('loop_empty')).render(*pose_np[-1])
    _check(out, g, m)
    launches, _, order = env.render_order()
    assert launches == k
    assert np.array_equal(np.sort(order), np.arange(n))
