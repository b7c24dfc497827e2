"""Exact-arithmetic inputs for the fp16 actor convolutions (aido1_amd/csrc/
dtconv.hip: dt_conv1_split, dt_conv32_split) and their float64 expectations.

The kernels multiply fp16 by fp16 into float32 accumulators and nothing is
contracted (-ffp-contract=off).  With the inputs, weights, bias, slope and the
incoming BatchNorm's (sc, sh) on a small dyadic grid, every staged input is
fp16-exact, every product and partial sum is exact in float32 in any order,
LeakyReLU (slope 1/4) is exact, and the stored value is the round-to-nearest-
even fp16 of an exactly known number: a float64 reference followed by
.float().half() equals the kernel's output bit for bit, and so does the centre.
tests/test_actor_exact_ref.py asserts those conditions on every pool;
tests/test_gpu_actor_exact.py runs the kernels.

A pool is P distinct samples of one layer; a launch of n samples gathers
pool[a[i]], so the expectation of any n is a gather too.

Grids (conv2..conv4): stored input integers in [-3, 3]; the previous layer's
statistics mean = k/4 (|k| <= 4) and M2 = IH IW sigma^2 with sigma in {1/2, 1,
2}, so with in_eps = 0 the kernel's M2 / cnt and sqrtf are exact; gamma in
{1/2, 1, 2}, beta = k/4: sc in [1/4, 4], sh on the 1/16 grid, staged |value|
<= 17 on the 1/16 grid.  Weights in {-1, 0, 1} with half of them zero, bias
k/4 (|k| <= 8), slope 1/4.  conv1: frames k/8 in [0, 1], weights k/4 (|k| <=
2), bias k/4.  Eval mode (prev_part = None, uncentred) takes the staged
values themselves as its fp16 input and a bias moved by an odd multiple of
1/32, so that the uncentred stored values exercise the store's rounding too.

Degenerate channels in every pool: output channels ZERO_CO have all-zero
weights and a bias of +1/4 and -1/4 (stored values exactly 0, statistics (0, 0,
c); conv4's own BatchNorm gives exactly fp16(out_beta)).  The `eps` variant of
a conv2..4 pool runs with in_eps = 1e-5: input channel FLAT_CI is flat in
every sample (x = 0, mean = 0, M2 = 0), so its sc = gamma / sqrt(eps) is not
dyadic and its staged value must still be exactly beta; the other channels'
M2 is moved to the float32 neighbour for which the kernel's float32
M2 / cnt + eps rounds to sigma^2 exactly, which keeps their (sc, sh) dyadic.

The statistics are not exact (Welford divides by 1, 2, 3, ...), so the module
also restates the kernels' accumulation order in float32: the per-lane Welford
over the lane's pixels in step order, the xor-butterfly Chan merge over the 32
lanes, the waves in order (welford32), and conv4's two-pass statistics with
its own BatchNorm (twopass32).  The GPU tests allow four times the error of
these restatements against float64 on the same pools, in the units below
(u = 2^-24):

  mean   |err| <= K u max|d|     d = v - c over the sample's channel
  M2     |err| <= K u M2
  conv4  |err| <= 2^-11 |want| + K u (|v| sc + mean|v| sc + |out_beta|)
         (the float32 mean's error goes with the mean of |v|, not with |mean|)

Measured on the pools the GPU tests use (VARIANTS; conv1 seeds 0 and 1),
worst case:

  layer   mean    M2      conv4
  1       0.79    2.56
  2       0.93    3.38
  3       0.64    2.36
  4                       3.18

K_STAT and K_OUT4 are four times those, rounded up.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

P = 7
SLOPE = 0.25
U = 2.0 ** -24
EPS = float(np.float32(1e-5))          # the float the kernels receive for 1e-5
# layer: IH, IW, OH, OW, stride, waves of the workgroup (tiles of 32 pixels a step)
GEOM = {1: (120, 160, 57, 77, 2, 4), 2: (57, 77, 27, 37, 2, 2), 3: (27, 37, 12, 17, 2, 2),
        4: (12, 17, 9, 14, 1, 4)}
ZERO_CO = (5, 22)      # all-zero weights; bias +1/4 and -1/4
FLAT_CI = 13           # flat input channel of the eps variant
TAP_GRAIN = 2.0 ** -6  # the sensitivity test's change of one weight tap

# the (seed, in_eps) pools of conv2..4 the GPU tests use: the first weight set,
# its flat-channel variant, the second weight set of the split launches
VARIANTS = ((0, 0.0), (0, 1e-5), (1, 0.0))

# 4 x the float32 restatements' worst error (module docstring), per layer
K_STAT = {1: (3.2, 10.3), 2: (3.8, 13.6), 3: (2.6, 9.5)}
K_OUT4 = 12.8


def lrelu(a):
    return torch.maximum(a, a * SLOPE)


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def tuned_m2(sigma2, cnt, eps):
    """The float32 M2 nearest cnt (sigma2 - eps) for which the kernel's
    float32 M2 / cnt + eps is exactly sigma2, or None where there is none (the
    eps variant then uses sigma = 1 instead)."""
    f = np.float32
    e, t, c = f(eps), f(sigma2), f(cnt)
    m = f((float(t) - float(e)) * cnt)
    lo = hi = m
    for _ in range(64):
        for cand in (lo, hi):
            if f(f(cand / c) + e) == t:
                return float(cand)
        lo, hi = np.nextafter(lo, f(0)), np.nextafter(hi, f(np.inf))
    return None       # M2's float32 spacing / cnt skips the window (conv2 at sigma 1/2)


def norm32(prev, gamma, beta, eps, cnt):
    """conv32_kernel's stats_merge in float32: (sc, sh) [P, 32] of each sample."""
    f = np.float32
    mean, m2 = prev[..., 0].astype(f), prev[..., 1].astype(f)
    with np.errstate(divide='ignore'):
        sc = gamma.astype(f) / np.sqrt(m2 / f(cnt) + f(eps))
    return sc, beta.astype(f) - mean * sc


def welford32(d, waves):
    """The kernels' statistics of d [P, C, pixels] (float32) in their order
    and precision: lane (wave, col) takes pixel 32 (waves j + wave) + col of
    step j, Welford over its pixels; the 32 lanes merge by xor butterfly (Chan),
    then the waves in order.  Returns (mean, M2) float32 [P, C]."""
    f = np.float32
    d = np.asarray(d, dtype=f)
    pn, ch, npix = d.shape
    tiles = -(-npix // 32)
    steps = -(-tiles // waves)
    pad = steps * waves * 32
    dp = np.zeros((pn, ch, pad), f)
    dp[..., :npix] = d
    dp = dp.reshape(pn, ch, steps, waves, 32)
    valid = (np.arange(pad) < npix).reshape(steps, waves, 32)
    cnt = np.zeros((1, 1, waves, 32), f)
    mean = np.zeros((pn, ch, waves, 32), f)
    m2 = np.zeros((pn, ch, waves, 32), f)
    for j in range(steps):
        vj = valid[j][None, None]
        v = dp[:, :, j]
        ncnt = cnt + vj.astype(f)
        inv = f(1) / np.maximum(ncnt, f(1))
        dd = v - mean
        nmean = mean + dd * inv
        nm2 = m2 + dd * (v - nmean)
        mean, m2, cnt = np.where(vj, nmean, mean), np.where(vj, nm2, m2), ncnt
    with np.errstate(divide='ignore', invalid='ignore'):
        for o in (1, 2, 4, 8, 16):
            idx = np.arange(32) ^ o
            nb = cnt[..., idx]
            tot = cnt + nb
            fa = np.where(tot > 0, nb / tot, f(0)).astype(f)
            fb = np.where(tot > 0, cnt * nb / tot, f(0)).astype(f)
            dd = mean[..., idx] - mean
            mean, m2, cnt = mean + dd * fa, m2 + (m2[..., idx] + dd * dd * fb), tot
    return _merge_waves(cnt[0, 0, :, 0], mean[..., 0], m2[..., 0])


def _merge_waves(cnt, mean, m2):
    """Chan's merge of the waves' (count [W], mean [P, C, W], M2) in order."""
    f = np.float32
    c = f(0)
    mu = np.zeros(mean.shape[:2], f)
    mm = np.zeros(mean.shape[:2], f)
    for w in range(len(cnt)):
        nb = f(cnt[w])
        if nb <= 0:
            continue
        tot = c + nb
        dd = mean[..., w] - mu
        mu = mu + dd * f(nb / tot)
        mm = mm + (m2[..., w] + dd * dd * f(f(c * nb) / tot))
        c = tot
    return mu, mm


def twopass32(v, gamma, beta, eps, waves=4):
    """conv4's epilogue (kOut 2) in float32: the two-pass statistics
    (twopass_stats32), sc = gamma / sqrt(M2 / pixels + eps), out = v sc +
    (beta - mean sc).  v [P, C, pixels] float32; returns float32 [P, C,
    pixels] before the fp16 rounding of the store."""
    f = np.float32
    v = np.asarray(v, dtype=f)
    mu, mm = twopass_stats32(v, waves)
    sc = gamma.astype(f) / np.sqrt(mm / f(v.shape[-1]) + f(eps))
    sh = beta.astype(f) - mu * sc
    return v * sc[..., None] + sh[..., None]


def twopass_stats32(v, waves=4):
    """conv4's two-pass statistics in float32: per wave the sum and then the
    M2 about its mean by xor butterflies (16, 8, .., 1), the waves merged in
    order.  v [P, C, pixels] float32; returns (mean, M2) float32 [P, C]."""
    f = np.float32
    v = np.asarray(v, dtype=f)
    pn, ch, npix = v.shape
    pad = waves * 32
    valid = (np.arange(pad) < npix).reshape(waves, 32)
    vp = np.zeros((pn, ch, pad), f)
    vp[..., :npix] = v
    vp = vp.reshape(pn, ch, waves, 32)

    def butterfly(s):
        for o in (16, 8, 4, 2, 1):
            s = s + s[..., np.arange(32) ^ o]
        return s
    nw = valid.sum(1).astype(f)                          # [W]
    inw = np.where(nw > 0, f(1) / np.maximum(nw, f(1)), f(0)).astype(f)
    mean_w = butterfly(np.where(valid, vp, f(0))) * inw[:, None]
    dd = np.where(valid, vp - mean_w, f(0))
    m2_w = butterfly(dd * dd)
    return _merge_waves(nw, mean_w[..., 0], m2_w[..., 0])


def _stats64(d):
    """float64 (mean, M2) of d [P, C, pixels]."""
    mean = d.mean(-1)
    return mean, ((d - mean[..., None]) ** 2).sum(-1)


def _finish(pool, layer, v, waves):
    """The reference-mode expectations of exact outputs v [P, 32, OH, OW]."""
    c = v[:, :, 0, 0].clone()
    d = v - c[:, :, None, None]
    pool.update(v=v, c=c, d=d, y=d.permute(0, 2, 3, 1).float().half().contiguous())
    dm = d.flatten(2)
    mean, m2 = _stats64(dm)
    pool.update(mean=mean, m2=m2, dmax=dm.abs().amax(-1))
    if layer != 4:
        m32, q32 = welford32(dm.numpy(), waves)
        pool.update(mean32=_t(m32), m2_32=_t(q32))
        pool['part'] = torch.stack([mean, m2, c], -1)      # float64 (mean, M2, c)


@functools.lru_cache(maxsize=None)
def pool32(layer, seed=0, eps=0.0):
    """P samples of conv layer 2..4 on the exact grids with every expectation
    (module docstring).  eps > 0: the flat-channel variant."""
    ih, iw, oh, ow, st, waves = GEOM[layer]
    rng = np.random.default_rng([layer, seed])
    x = rng.integers(-3, 4, (P, ih, iw, 32)).astype(np.float64)
    mean = rng.integers(-4, 5, (P, 32)) / 4.0
    sigma = rng.choice([0.5, 1.0, 2.0], (P, 32))
    gamma = rng.choice([0.5, 1.0, 2.0], 32)
    beta = rng.integers(-4, 5, 32) / 4.0
    w = (rng.integers(-1, 2, (32, 32, 4, 4)) * (rng.random((32, 32, 4, 4)) < 0.5)).astype(
        np.float64)
    b = rng.integers(-8, 9, 32) / 4.0
    og = rng.choice([0.5, 1.0, 2.0], 32)
    ob = rng.integers(-4, 5, 32) / 4.0
    for co, sign in zip(ZERO_CO, (1.0, -1.0)):
        w[co] = 0.0
        b[co] = 0.25 * sign
        ob[co] = 0.5 * sign
    cnt = ih * iw
    m2 = cnt * sigma ** 2
    if eps:
        tuned = {s: tuned_m2(s * s, cnt, eps) for s in (0.5, 1.0, 2.0)}
        assert tuned[1.0] is not None
        sigma = np.where(np.isin(sigma, [s for s in tuned if tuned[s] is None]), 1.0, sigma)
        m2 = np.vectorize(tuned.get)(sigma).astype(np.float64)
        x[..., FLAT_CI] = 0.0
        mean[:, FLAT_CI] = 0.0
        m2[:, FLAT_CI] = 0.0
    prev = np.stack([mean, m2, np.zeros_like(mean)], -1).astype(np.float32)
    sc, sh = norm32(prev, gamma, beta, eps, cnt)
    # the kernel's fma of the fp16 input, exact in float64 (3 x 24 bits)
    staged = x * sc.astype(np.float64)[:, None, None, :] + sh.astype(np.float64)[:, None, None, :]
    pool = dict(layer=layer, eps=float(eps), x16=_t(x, torch.float16), prev=_t(prev, torch.float32),
                gamma=_t(gamma, torch.float32), beta=_t(beta, torch.float32),
                w=_t(w, torch.float32), b=_t(b, torch.float32), og=_t(og, torch.float32),
                ob=_t(ob, torch.float32), sc=_t(sc), sh=_t(sh), staged=_t(staged))
    wt, bt = _t(w), _t(b)
    xs = pool['staged'].permute(0, 3, 1, 2)
    acc = F.conv2d(xs, wt, bt, stride=st)
    pool['acc'] = acc
    pool['terms'] = F.conv2d(xs.abs(), wt.abs(), bt.abs(), stride=st)
    _finish(pool, layer, lrelu(acc), waves)
    if layer == 4:                       # its own BatchNorm, flattened NCHW
        v = pool['v'].flatten(2)
        mu, mm = _stats64(v)
        s64 = _t(og) / torch.sqrt(mm / v.shape[-1] + EPS)
        pool['want'] = (v * s64[..., None] + (_t(ob) - mu * s64)[..., None]).flatten(1)
        pool['unit'] = (v.abs() * s64[..., None] +
                        (v.abs().mean(-1) * s64 + _t(ob).abs())[..., None]).flatten(1)
        pool['out32'] = _t(twopass32(v.numpy(), og, ob, EPS, waves)).flatten(1)
    if not eps:
        # eval mode (no input norm, uncentred): the staged values themselves as
        # the fp16 input and a bias on the 1/32 grid, so that the uncentred
        # values also exercise the store's rounding
        be = b + rng.choice([-3, -1, 1, 3], 32) / 32.0
        be[list(ZERO_CO)] = b[list(ZERO_CO)]
        pool['xe16'] = pool['staged'].half().contiguous()
        pool['be'] = _t(be, torch.float32)
        pool['acce'] = acc + _t(be - b)[None, :, None, None]
        ve = pool['ve'] = lrelu(pool['acce'])
        pool['ye'] = (ve.flatten(1) if layer == 4 else ve.permute(0, 2, 3, 1)).float().half(
        ).contiguous()
    return pool


@functools.lru_cache(maxsize=None)
def pool1(seed=0):
    """P samples of conv1: frames [P, 3, 120, 160] oldest first (float32,
    k/8), weights, bias and the expectations with and without statistics."""
    ih, iw, oh, ow, st, waves = GEOM[1]
    rng = np.random.default_rng([1, seed])
    frames = rng.integers(0, 9, (P, 3, ih, iw)) / 8.0
    w = rng.integers(-2, 3, (32, 3, 8, 8)) / 4.0
    b = rng.integers(-8, 9, 32) / 4.0
    for co, sign in zip(ZERO_CO, (1.0, -1.0)):
        w[co] = 0.0
        b[co] = 0.25 * sign
    pool = dict(layer=1, frames=_t(frames, torch.float32), w=_t(w, torch.float32),
                b=_t(b, torch.float32), staged=_t(frames))
    acc = F.conv2d(_t(frames), _t(w), _t(b), stride=st)
    pool['acc'] = acc
    pool['terms'] = F.conv2d(_t(frames), _t(w).abs(), _t(b).abs(), stride=st)
    _finish(pool, 1, lrelu(acc), waves)
    pool['ye'] = pool['v'].permute(0, 2, 3, 1).float().half().contiguous()
    return pool


def stat_units(pool):
    """The float32 restatement's worst statistics error in the units of the
    bounds: (mean, M2).  Where the unit is 0 (a flat channel) the restatement
    must be exact."""
    out = []
    for got, ref, unit in ((pool['mean32'], pool['mean'], pool['dmax']),
                           (pool['m2_32'], pool['m2'], pool['m2'])):
        err = (got - ref).abs()
        assert bool((err[unit == 0] == 0).all())
        nz = unit > 0
        out.append((err[nz] / (U * unit[nz])).max().item())
    return tuple(out)


def out4_units(pool):
    """The float32 restatement of conv4's normalised output against float64,
    in units of u (|v| sc + mean|v| sc + |out_beta|)."""
    return ((pool['out32'] - pool['want']).abs() / (U * pool['unit'])).max().item()


def perturbed_tap(pool, co=9, ci=3, ky=1, kx=2):
    """The weights with tap (co, ci, ky, kx) raised by TAP_GRAIN, and the
    exact reference-mode outputs v they give: the sensitivity test's error."""
    st = GEOM[pool['layer']][4]
    w = pool['w'].clone()
    w[co, ci, ky, kx] += TAP_GRAIN
    v = lrelu(F.conv2d(pool['staged'].permute(0, 3, 1, 2), w.double(), pool['b'].double(),
                       stride=st))
    return w, v
