"""The fused render kernel at the frame's clamped edges: 64 poses all over
loop_empty whose frames have non-uniform words in every border row and column
and in every corner word (asserted on the oracle's frames before anything is
compared), so the uniformity test's clamped side words, the rounds only some
waves run, Sobel's BORDER_REPLICATE and the NMS neighbours outside the image
all decide bits.  Grey and the four masks bit for bit against the C oracle
(oracle/render_oracle.c), per dilation size, frame format and list cap, and a
three-decision group against three single renders.  The host-only test restates
the uniformity test's pair-difference form in numpy against the per-pixel
definition."""
import functools
import math

import numpy as np
import pytest

from conftest import map_rows
from oracle import oracle_c as OC

N = 64          # below the 512-env threshold: the dispatch order is the identity
TS = 0.585
H, W, WPR = 120, 160, 40


def edge_poses():
    rng = np.random.default_rng(20261021)
    x = rng.uniform(0.2, 3 * TS - 0.2, N)
    z = rng.uniform(0.2, 3 * TS - 0.2, N)
    a = rng.uniform(-math.pi, math.pi, N)
    return x, z, a


def nonuniform_words(frames):
    """[n, 120, 40] bool: the 3 x 6 pixels around a 4-pixel word (edge pixels
    replicated) are not one value; frames [n, 120, 160] of any dtype."""
    p = np.pad(frames, ((0, 0), (1, 1), (1, 1)), mode='edge')
    out = np.zeros((frames.shape[0], H, WPR), bool)
    for cw in range(WPR):
        blk = np.stack([p[:, dr:dr + H, 4 * cw + dc] for dr in range(3) for dc in range(6)], -1)
        out[:, :, cw] = (blk != blk[..., :1]).any(-1)
    return out


@functools.lru_cache(maxsize=None)
def reference(dil=None):
    """The oracle's (grey, masks) of the edge poses, computed once per
    parameter set; the default set also proves the poses reach the edges."""
    x, z, a = edge_poses()
    p = OC.line_params_default()
    if dil is not None:
        p.dilation_kernel_size = dil
    g, m, rgb = OC.OracleRender(map_rows('loop_empty'), params=p).render(x, z, a)
    if dil is None:
        col = rgb[..., 0].astype(np.int32) | (rgb[..., 1].astype(np.int32) << 8) | \
            (rgb[..., 2].astype(np.int32) << 16)
        nu = nonuniform_words(col)
        assert int(nu[:, 0].any(1).sum()) == 27          # frames with a listed word in the top row
        assert int(nu[:, -1].any(1).sum()) == 64         # ... the bottom row
        assert int(nu[:, :, 0].any(1).sum()) == 43       # ... the left word column
        assert int(nu[:, :, -1].any(1).sum()) == 47      # ... the right one
        for r, c in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
            assert int(nu[:, r, c].sum()) >= 2           # every corner word
        cnt = nu.reshape(N, -1).sum(1)
        assert (int(cnt.min()), int(cnt.max()), float(np.median(cnt))) == (205, 1307, 917.0)
    g.setflags(write=False)
    m.setflags(write=False)
    return g, m


def make_env(gpu):
    from aido1_amd.vec_env import VecEnv
    env = VecEnv(N, seed=31)
    env.reset()
    x, z, a = edge_poses()
    env.set_state(x=x, z=z, angle=a)
    return env


@pytest.mark.gpu
@pytest.mark.parametrize('dil', [None, 3, 5, 7])
def test_edges_match_oracle(gpu, dil):
    """The default parameters, and dilation kernel sizes 3 (the radius-1 path)
    and 5, 7 (the radius 2-3 kernels, which share phases 1 to 2b)."""
    import torch
    from aido1_amd.render import LineParams, RenderOutput
    g, m = reference(dil)
    env = make_env(gpu)
    if dil is not None:
        lp = LineParams.default()
        lp.dilation_kernel_size = dil
        env.set_line_params(lp)
    out = RenderOutput(N, gpu, slots=1)
    env.render_into(out)
    torch.cuda.synchronize()
    assert np.array_equal(out.masks.cpu().numpy(), m)
    assert np.array_equal(out.ring[:, 0].cpu().numpy(), g)


@pytest.mark.gpu
def test_edges_index_frames(gpu):
    """Palette-index frames, decoded through the grey table."""
    import torch
    from aido1_amd.render import RenderOutput, decode_index
    g, m = reference()
    env = make_env(gpu)
    out = RenderOutput(N, gpu, slots=1, frames='index')
    env.render_into(out)
    torch.cuda.synchronize()
    assert out.ring.dtype == torch.uint8 and int(out.ring.max()) <= 7
    assert np.array_equal(out.masks.cpu().numpy(), m)
    assert np.array_equal(decode_index(out.ring[:, 0]).cpu().numpy(), g)


@pytest.mark.gpu
@pytest.mark.parametrize('list_cap', [1, 64, 700])
def test_edges_list_cap(gpu, list_cap):
    """The spill kernels and the list stores' cap test: the frames list 205 to
    1,307 words, so every cap has waves whose slots straddle it."""
    import torch
    from aido1_amd.render import RenderOutput
    g, m = reference()
    env = make_env(gpu)
    out = RenderOutput(N, gpu, slots=1)
    env.render_into(out, list_cap=list_cap)
    torch.cuda.synchronize()
    assert np.array_equal(out.masks.cpu().numpy(), m)
    assert np.array_equal(out.ring[:, 0].cpu().numpy(), g)


@pytest.mark.gpu
def test_edges_render3_group(gpu):
    """dt_render3 over three consecutive decisions from the edge poses, fresh
    flags set in the middle one, against three single renders."""
    import torch
    from aido1_amd.render import RenderOutput, render_group_into
    reference()   # the poses reach the edges
    env = make_env(gpu)
    ref = RenderOutput(N, gpu)
    grp = RenderOutput(N, gpu)
    extra = [torch.zeros_like(grp.masks) for _ in range(2)]
    gen = torch.Generator(device=gpu)
    gen.manual_seed(9)
    poses, fresh, want = [], [], []
    for k in range(3):
        p = torch.empty(3, N, dtype=torch.float64, device=gpu)
        env.copy_pose(p)
        poses.append(p)
        f = torch.rand(N, generator=gen, device=gpu) < 0.3 if k == 1 else \
            torch.zeros(N, dtype=torch.bool, device=gpu)
        fresh.append(f.to(torch.uint8))
        env.step_into(torch.rand(N, 2, generator=gen, device=gpu))
    assert int(fresh[1].sum()) > 0
    for f, p in zip(fresh, poses):
        env.render_into(ref, fresh=f, pose=p)
        want.append(ref.masks.clone())
    render_group_into(env, grp, extra, fresh, poses)
    torch.cuda.synchronize()
    assert grp.slot == ref.slot
    for got, w in zip([grp.masks] + extra, want):
        assert torch.equal(got, w)
    assert torch.equal(grp.ring, ref.ring)
    # decision 0 is the edge poses themselves: the oracle's masks
    assert np.array_equal(grp.masks.cpu().numpy(), reference()[1])


def _alignbyte1(hi, lo):
    """v_alignbyte(hi, lo, 1): bytes 1-3 of lo below byte 0 of hi."""
    return ((lo >> np.uint32(8)) | (hi << np.uint32(24))).astype(np.uint32)


def test_pair_difference_uniformity_is_the_per_pixel_one():
    """Phase 1's test of a 16-pixel quad by pair differences (V, A, diff, as
    render_env computes them on the six words of three rows) against the
    definition: a word is uniform iff the 3 x 6 pixels around it are one byte.
    Random rows of few colours, with runs, so both answers occur at every
    byte position; the clamped side words (the quad's own edge word) included."""
    rng = np.random.default_rng(5)
    n = 200000
    # three rows of 24 pixels: mostly one colour, with a few runs of others
    px = np.repeat(rng.integers(0, 8, (n, 1, 1), dtype=np.uint8), 3, 1).repeat(24, 2)
    for _ in range(2):
        r0 = rng.integers(0, 3, n)
        c0 = rng.integers(0, 24, n)
        ln = rng.integers(1, 6, n)
        col = rng.integers(0, 8, n, dtype=np.uint8)
        hit = rng.random(n) < 0.6
        cols = np.arange(24)[None, :]
        msk = hit[:, None] & (cols >= c0[:, None]) & (cols < (c0 + ln)[:, None])
        for r in range(3):
            rows = msk & (r0 <= r)[:, None] & (rng.random(n) < 0.8)[:, None]
            px[:, r][rows] = np.broadcast_to(col[:, None], (n, 24))[rows]
    for edge in ('none', 'left', 'right'):
        p = px.copy()
        if edge == 'left':     # the side word is the quad's own first word
            p[:, :, 0:4] = p[:, :, 4:8]
        if edge == 'right':
            p[:, :, 20:24] = p[:, :, 16:20]
        w = p.reshape(n, 3, 6, 4).astype(np.uint32)
        w = w[..., 0] | (w[..., 1] << 8) | (w[..., 2] << 16) | (w[..., 3] << 24)   # [n, 3, 6]
        V = (w[:, 0] ^ w[:, 1]) | (w[:, 1] ^ w[:, 2])
        A = V[:, :5] | (w[:, 1, :5] ^ _alignbyte1(w[:, 1, 1:], w[:, 1, :5]))
        for j in range(4):
            diff = A[:, j + 1] | (A[:, j] & np.uint32(0xFF000000)) | (V[:, j + 2] & np.uint32(0xFF))
            # the definition, with the image edge's replicated pixel
            lo, hi = 4 * (j + 1) - 1, 4 * (j + 1) + 5
            blk = p[:, :, lo:hi].copy()
            if edge == 'left' and j == 0:
                blk[:, :, 0] = blk[:, :, 1]
            if edge == 'right' and j == 3:
                blk[:, :, 5] = blk[:, :, 4]
            want = (blk.reshape(n, -1) != blk[:, 1, 1][:, None]).any(1)
            got = diff != 0
            assert np.array_equal(got, want), (edge, j)
            assert want.any() and not want.all()
