"""Exact-arithmetic inputs for the float32-accurate "x3" actor kernels
(aido1_amd/csrc/dtconvx.hip: dt_conv1x_split, dt_conv32x_split,
dt_actor_head_x3) and their float64 expectations, on top of the fp16 chain's
tests/actor_exact_ref.py (GEOM, P, ZERO_CO, FLAT_CI, tuned_m2, norm32,
welford32 and the pool-and-gather scheme are its own).

The arithmetic model.  Every f32 operand t is an fp16 pair, hi = fp16(t), lo =
fp16((t - hi) 2^11); the kernels accumulate acc0 = sum ah bh and acc1 = sum
(ah bl + al bh) in float32 and combine v = lrelu((acc0 + acc1 2^-11) 2^e +
bias'), nothing contracted.  For conv2..4 the A operand is the folded weight
w' = w sc 2^-e (sc, sh the previous layer's per-sample BatchNorm; e > 0 only
where max|sc| max|w| > 16384), bias' = bias + sum w sh; for conv1 and lin1 it
is the weight itself and e = 0.  On the grids below every operand equals hi +
2^-11 lo exactly, every product, every partial sum of either accumulator in
any order, the combination, w', bias' in any order and LeakyReLU (slope 1/4)
are exact in float32, so three float64 conv2d calls, one a product, give the
kernel's v exactly, and the store's own split of v - c gives the bits.  Both
inputs and weights carry lo != 0 in about half of their non-zero elements, so
the dropped al bl 2^-22 is not zero: the model is the reference, and
tests/test_actor_x3_exact_ref.py asserts that it is within 2^-22 sum |a||b| of
the true float64 convolution, with every other condition named here.

Grids.  conv2..conv4: x = k + f 2^-13, k in [-2, 2], f in {-1, 0, 1} (0 where
k = 0): hi = k, lo = f / 4.  Previous statistics mean = k / 4 (|k| <= 2), M2 =
IH IW sigma^2, sigma in {1/2, 1, 2}, gamma in {1/2, 1, 2}, beta = k / 4; where
sc = gamma / sigma < 1 the mean is k / (4 sc), so that sh = beta - mean sc and
with it bias' stay on grids no finer than the products'.  v - c is NOT always
a float32 number (|v| reaches 170 on the 2^-17 grid of a negative value): the
kernel rounds it once and so does the reference, before the split.
Weights a + b 2^-13, a in {-1, 0, 1} (a quarter of them non-zero, which keeps
the sums inside 24 bits of their finest term), b in {-1, 0, 1}: 14 significant
bits, and so after the fold by a power of two.  conv1: frames k / 8 + f 2^-13
with k in {0, 4..8} (hi's ulp there is 2^-11, so lo = f / 4), weights a / 4 +
b 2^-15, |a| <= 2.  lin1: x = k + f 2^-13 (|k| <= 1), w1 = a + b 2^-13 (a
quarter non-zero); lin2's w2 has W2_TAPS entries of +-1 a row, so that its
sums of the 2^-15-grained hidden values stay exact in any order, and lin1 is
seen through the kernel's own partial sums (the `work` buffer of
include/dtactor.h: [4 K quarters][512 features][n]) as well as through the
output.

Variants of a conv2..4 pool:
  plain    the grids above; seed 1 is the second weight set of split launches
  eps      in_eps = 1e-5: input channel FLAT_CI flat in every sample (x = 0,
           mean = 0, M2 = 0), its weights non-zero in every tap: sc = gamma /
           sqrt(eps) is not dyadic, w' is rounded, and its contribution must
           still be exactly sum w beta; tuned_m2 keeps the other channels dyadic
  rescale  input channel RS_CI has gamma 2^16, sigma 2 and weights a 2^-12:
           max|sc| max|w| = 2^15 (1 + 2^-13), e = 2; sample RS_OFF has sigma 16
           there and e = 0 (the scale is per sample)
  subw     input channel SW_CI has sigma 2^10, x = 2^10 k and weights a 2^-6:
           w' = a 2^-16, an fp16 subnormal hi half
  sublo    a quarter of the (sample, channel) pairs scaled by 2^-14 (x, mean,
           sigma): lo = f 2^-16, an fp16 subnormal, hi down to 2^-14, sc up to
           2^16 (so e up to 3); the products are those of the plain pool

The statistics divide, so they are restated in float32 (welford32 on four
waves; conv4's two-pass statistics and x3's own (v - mean) sc + beta) and the
kernels are allowed four times the restatement's worst error against float64,
in the units of actor_exact_ref (u = 2^-24):

  mean   |err| <= K u max|d|
  M2     |err| <= K u M2
  conv4  |err| <= K u (|v| sc + mean|v| sc + |out_beta|)     (f32 store)

Measured over every pool the GPU tests use (VARIANTS32X; conv1 seeds 0, 1):

  layer   mean    M2      conv4
  1       0.68    2.86
  2       1.13    3.10
  3       0.85    2.29
  4                       3.17

K_STAT and K_OUT4 are four times those, rounded up.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import actor_exact_ref as R
from actor_exact_ref import EPS, FLAT_CI, GEOM, P, SLOPE, U, ZERO_CO, _t, lrelu  # noqa: F401

WAVES = 4                  # every x3 convolution kernel runs four waves a workgroup
LO = 2048.0
RS_CI, RS_OFF = 7, 2       # the rescale variant's channel; its sample without a rescale
SW_CI = 21                 # the subnormal-weight variant's channel
DENSITY = 0.25             # share of non-zero weights
W2_TAPS = 12               # non-zero entries a row of lin2
LO_GRAIN = 2.0 ** -13      # one grain of a weight's lo half (conv2..4, lin1)
# stride at which each layer's consumer reads its HLB output (conv4 stores f32)
NEXT_STRIDE = {1: 2, 2: 2, 3: 1}

# (seed, variant) pools of conv2..4 the GPU tests use
VARIANTS32X = ((0, 'plain'), (0, 'eps'), (1, 'plain'), (0, 'rescale'), (0, 'subw'), (0, 'sublo'))

# 4 x the float32 restatements' worst error (module docstring), per layer
K_STAT = {1: (2.8, 11.5), 2: (4.6, 12.4), 3: (3.4, 9.2)}
K_OUT4 = 12.7


def split16(t):
    """The kernels' split of float32 values t (numpy): (hi, lo) as float16."""
    t = np.asarray(t, dtype=np.float32)
    hi = t.astype(np.float16)
    return hi, ((t - hi.astype(np.float32)) * np.float32(LO)).astype(np.float16)


def grain(a):
    """The largest power of two of which every element of a is a multiple
    (inf for all zeros): elements m 2^e with m odd -> min 2^e."""
    a = np.abs(np.asarray(a, dtype=np.float64)).ravel()
    a = a[a != 0]
    if a.size == 0:
        return np.inf
    m, e = np.frexp(a)
    m = (m * 2.0 ** 53).astype(np.int64)
    low = (m & -m).astype(np.float64)
    return float((np.ldexp(low, e - 53)).min())


def _gconv(x, w, st):
    """Per-sample weights: x [P, C, H, W], w [P, Co, C, kh, kw] (float64)."""
    pn, c = x.shape[:2]
    out = F.conv2d(x.reshape(1, pn * c, *x.shape[2:]), w.reshape(-1, *w.shape[2:]), stride=st,
                   groups=pn)
    return out.reshape(pn, w.shape[1], *out.shape[2:])


def model3(xh, xl, ah, al, st):
    """The three-product model on float64 halves: acc0, acc1 and the sums of
    their terms' magnitudes.  x [P, C, H, W], a [P, Co, C, kh, kw]."""
    acc0 = _gconv(xh, ah, st)
    acc1 = _gconv(xl, ah, st) + _gconv(xh, al, st)
    t0 = _gconv(xh.abs(), ah.abs(), st)
    t1 = _gconv(xl.abs(), ah.abs(), st) + _gconv(xh.abs(), al.abs(), st)
    return acc0, acc1, t0, t1


def hlb_image(d32, stride, fill):
    """float32 [n, h, w, 32] -> the kernel's HLB store of it as int16 bits [n,
    h, 4, 2, chunks, 8], the chunks no pixel owns holding `fill`."""
    from aido1_amd.actor import hlb_geometry
    n, h, w, _ = d32.shape
    segpx, pos = hlb_geometry(w, stride)
    hi = d32.half()
    lo = ((d32 - hi.float()) * LO).half()
    pair = torch.stack([hi, lo]).view(torch.int16).reshape(2, n, h, w, 4, 8).permute(1, 2, 4, 0, 3, 5)
    out = torch.full((n, h, 4, 2, segpx, 8), fill, dtype=torch.int16, device=d32.device)
    out[:, :, :, :, pos, :] = pair
    return out


def _finish(pool, layer, v):
    """The expectations of exact outputs v [P, 32, OH, OW] (float64)."""
    c = v[:, :, 0, 0].clone()
    d = v - c[:, :, None, None]
    pool.update(v=v, c=c, d=d)
    dm = d.flatten(2)
    mean, m2 = R._stats64(dm)
    pool.update(mean=mean, m2=m2, dmax=dm.abs().amax(-1))
    if layer != 4:
        pool['d32'] = d.permute(0, 2, 3, 1).float().contiguous()      # NHWC, the stored value
        m32, q32 = R.welford32(dm.float().numpy(), WAVES)
        pool.update(mean32=_t(m32), m2_32=_t(q32))
        pool['part'] = torch.stack([mean, m2, c], -1)
        return
    og, ob = pool['og'].double(), pool['ob'].double()
    vf = v.flatten(2)
    mu, mm = R._stats64(vf)
    s64 = og / torch.sqrt(mm / vf.shape[-1] + EPS)
    pool['want'] = ((vf - mu[..., None]) * s64[..., None] + ob[..., None]).flatten(1)
    pool['unit'] = (vf.abs() * s64[..., None] +
                    (vf.abs().mean(-1) * s64 + ob.abs())[..., None]).flatten(1)
    f = np.float32
    v32 = vf.float().numpy()
    mu32, mm32 = R.twopass_stats32(v32, WAVES)
    sc32 = pool['og'].numpy() / np.sqrt(mm32 / f(v32.shape[-1]) + f(EPS))
    out32 = (v32 - mu32[..., None]) * sc32[..., None] + pool['ob'].numpy()[..., None]
    pool['out32'] = _t(out32).flatten(1)


def fold32(w, sc):
    """conv32x_kernel's fold in float32: the per-sample exponent e [P] and the
    folded weights w sc 2^-e [P, 32, 32, 4, 4] as the kernel rounds them."""
    f = np.float32
    w, sc = np.asarray(w, dtype=f), np.asarray(sc, dtype=f)
    wmax = np.abs(w).max()
    bound = np.abs(sc).max(1) * wmax
    e = np.zeros(sc.shape[0], np.int64)
    big = (bound > f(16384)) & np.isfinite(bound)
    e[big] = np.frexp(bound[big] * f(1.0 / 16384))[1]
    wsc = np.ldexp(f(1), -e).astype(f)
    t = (w[None] * sc[:, None, :, None, None]) * wsc[:, None, None, None, None]
    return e, t.astype(f)


@functools.lru_cache(maxsize=None)
def pool32x(layer, seed=0, variant='plain', kmax=2):
    """P samples of conv layer 2..4 on the exact grids with every expectation
    and the intermediates the host test checks (module docstring).  kmax: the
    inputs' range (the host test widens it to see its checks fail)."""
    from aido1_amd.actor import hlb_encode
    ih, iw, oh, ow, st, _ = GEOM[layer]
    rng = np.random.default_rng([layer, seed, 3])
    k = rng.integers(-kmax, kmax + 1, (P, ih, iw, 32)).astype(np.float64)
    fl = rng.integers(-1, 2, k.shape) * (k != 0)
    x = k + fl * LO_GRAIN
    mean = rng.integers(-2, 3, (P, 32)) / 4.0
    sigma = rng.choice([0.5, 1.0, 2.0], (P, 32))
    gamma = rng.choice([0.5, 1.0, 2.0], 32)
    beta = rng.integers(-4, 5, 32) / 4.0
    # on the k / 4 grid, and coarse enough that sh = beta - mean sc is on it too
    mean = mean * np.maximum(1.0, sigma / gamma)
    a = rng.choice([-1.0, 1.0], (32, 32, 4, 4)) * (rng.random((32, 32, 4, 4)) < DENSITY)
    b = rng.integers(-1, 2, a.shape) * (a != 0)
    dense_a = rng.choice([-1.0, 1.0], a.shape)       # for the channels that are non-zero in every tap
    bias = rng.integers(-8, 9, 32) / 4.0
    og = rng.choice([0.5, 1.0, 2.0], 32)
    ob = rng.integers(-4, 5, 32) / 4.0
    tiny = rng.random((P, 32)) < 0.25
    eps = 0.0
    cnt = ih * iw
    w = a + b * LO_GRAIN
    if variant == 'eps':
        eps = 1e-5
        tuned = {s: R.tuned_m2(s * s, cnt, eps) for s in (0.5, 1.0, 2.0)}
        assert tuned[1.0] is not None
        sigma = np.where(np.isin(sigma, [s for s in tuned if tuned[s] is None]), 1.0, sigma)
        m2 = np.vectorize(tuned.get)(sigma).astype(np.float64)
        x[..., FLAT_CI] = 0.0
        mean[:, FLAT_CI] = 0.0
        m2[:, FLAT_CI] = 0.0
        w[:, FLAT_CI] = dense_a[:, FLAT_CI] + b[:, FLAT_CI] * LO_GRAIN
        if beta[FLAT_CI] == 0:
            beta[FLAT_CI] = 0.75
    elif variant == 'rescale':
        gamma[RS_CI] = 2.0 ** 16
        sigma[:, RS_CI] = 2.0
        sigma[RS_OFF, RS_CI] = 16.0
        mean[:, RS_CI] = 0.0
        w[:, RS_CI] = a[:, RS_CI] * 2.0 ** -12
        if beta[RS_CI] == 0:
            beta[RS_CI] = -0.5
    elif variant == 'subw':
        gamma[SW_CI] = 1.0
        sigma[:, SW_CI] = 2.0 ** 10
        x[..., SW_CI] = k[..., SW_CI] * 2.0 ** 10
        mean[:, SW_CI] = mean[:, SW_CI] * 2.0 ** 10
        w[:, SW_CI] = dense_a[:, SW_CI] * 2.0 ** -6
    elif variant == 'sublo':
        s = np.where(tiny, 2.0 ** -14, 1.0)
        x = x * s[:, None, None, :]
        mean = mean * s
        sigma = sigma * s
    else:
        assert variant == 'plain', variant
    if variant != 'eps':
        m2 = cnt * sigma ** 2
    for co, sign in zip(ZERO_CO, (1.0, -1.0)):
        w[co] = 0.0
        bias[co] = 0.25 * sign
        ob[co] = 0.5 * sign
    prev = np.stack([mean, m2, np.zeros_like(mean)], -1).astype(np.float32)
    sc, sh = R.norm32(prev, gamma, beta, eps, cnt)
    e, t32 = fold32(w, sc)
    th, tl = split16(t32)
    xh, xl = split16(x)
    x32 = _t(x, torch.float32)
    pool = dict(layer=layer, variant=variant, eps=float(eps), x=_t(x),
                xin=hlb_encode(x32, st).contiguous(), prev=_t(prev, torch.float32),
                gamma=_t(gamma, torch.float32), beta=_t(beta, torch.float32),
                w=_t(w, torch.float32), w64=_t(w), b=_t(bias, torch.float32),
                og=_t(og, torch.float32), ob=_t(ob, torch.float32), sc=_t(sc), sh=_t(sh),
                e=torch.from_numpy(e), t32=_t(t32), th=_t(th), tl=_t(tl), xh=_t(xh), xl=_t(xl))
    nchw = (lambda q: _t(q).permute(0, 3, 1, 2))
    acc0, acc1, t0, t1 = model3(nchw(xh), nchw(xl), pool['th'], pool['tl'], st)
    # bias' = bias + sum w sh: its terms [P, 32, 512] (exact in float64: 24 x 24 bits)
    bterms = (pool['w64'][None] * pool['sh'][:, None, :, None, None]).flatten(2)
    b2 = _t(bias)[None] + bterms.sum(-1)
    comb = acc0 + acc1 / LO
    pre = comb * torch.ldexp(torch.ones(P, dtype=torch.float64), pool['e'])[:, None, None, None] + \
        b2[:, :, None, None]
    pool.update(acc0=acc0, acc1=acc1, t0=t0, t1=t1, comb=comb, bterms=bterms, b2=b2, pre=pre)
    # the true float64 convolution of the same operands, for the dropped al bl
    pool['true'] = _gconv(nchw(x), pool['t32'], st)
    pool['true_abs'] = _gconv(nchw(x).abs(), pool['t32'].abs(), st)
    _finish(pool, layer, lrelu(pre))
    return pool


@functools.lru_cache(maxsize=None)
def pool1x(seed=0):
    """P samples of conv1: grey frames [P, 3, 120, 160] oldest first, weights,
    bias and the expectations."""
    ih, iw, oh, ow, st, _ = GEOM[1]
    rng = np.random.default_rng([1, seed, 3])
    k = rng.choice([0, 4, 5, 6, 7, 8], (P, 3, ih, iw)).astype(np.float64)
    fl = rng.integers(-1, 2, k.shape) * (k != 0)
    fl = np.where((k == 8) & (fl > 0), 0, fl)
    frames = k / 8.0 + fl * LO_GRAIN
    a = rng.integers(-2, 3, (32, 3, 8, 8)).astype(np.float64)
    b = rng.integers(-1, 2, a.shape) * (a != 0)
    w = a / 4.0 + b * 2.0 ** -15
    bias = rng.integers(-8, 9, 32) / 4.0
    for co, sign in zip(ZERO_CO, (1.0, -1.0)):
        w[co] = 0.0
        bias[co] = 0.25 * sign
    wh, wl = split16(w)
    xh, xl = split16(frames)
    pool = dict(layer=1, frames=_t(frames, torch.float32), x=_t(frames), w=_t(w, torch.float32),
                w64=_t(w), b=_t(bias, torch.float32), th=_t(wh)[None], tl=_t(wl)[None],
                xh=_t(xh), xl=_t(xl))
    ah, al = _t(wh).expand(P, -1, -1, -1, -1), _t(wl).expand(P, -1, -1, -1, -1)
    acc0, acc1, t0, t1 = model3(_t(xh), _t(xl), ah, al, st)
    bb = _t(bias)[None, :, None, None]
    acc0, t0 = acc0 + bb, t0 + bb.abs()             # acc0 starts at the bias
    comb = acc0 + acc1 / LO
    pool.update(acc0=acc0, acc1=acc1, t0=t0, t1=t1, comb=comb, pre=comb)
    pool['true'] = F.conv2d(_t(frames), _t(w), _t(bias), stride=st)
    pool['true_abs'] = F.conv2d(_t(frames).abs(), _t(w).abs(), _t(bias).abs(), stride=st)
    _finish(pool, 1, lrelu(comb))
    return pool


@functools.lru_cache(maxsize=None)
def pool_head(seed=0):
    """P rows of lin1's input [P, 4032] with the head's parameters and the
    float64 model of dt_actor_head_x3 at head code 0: the four K quarters'
    partial sums, the hidden values and the output [P, 2]."""
    rng = np.random.default_rng([5, seed, 3])
    k = rng.integers(-1, 2, (P, 4032)).astype(np.float64)
    fl = rng.integers(-1, 2, k.shape) * (k != 0)
    x = k + fl * LO_GRAIN
    a = rng.choice([-1.0, 1.0], (512, 4032)) * (rng.random((512, 4032)) < DENSITY)
    b = rng.integers(-1, 2, a.shape) * (a != 0)
    w1 = a + b * LO_GRAIN
    b1 = rng.integers(-8, 9, 512) / 4.0
    w2 = np.zeros((2, 512))
    for j in range(2):
        taps = rng.choice(512, W2_TAPS, replace=False)
        w2[j, taps] = rng.choice([-1.0, 1.0], W2_TAPS)
    b2 = rng.integers(-8, 9, 2) / 4.0
    wh, wl = split16(w1)
    xh, xl = split16(x)
    pool = dict(x=_t(x, torch.float32), x64=_t(x), w1=_t(w1, torch.float32), w1_64=_t(w1),
                b1=_t(b1, torch.float32), w2=_t(w2, torch.float32), b2=_t(b2, torch.float32),
                xh=_t(xh), xl=_t(xl), th=_t(wh), tl=_t(wl))
    q = (lambda t: t.reshape(t.shape[0], 4, 1008))
    xhq, xlq, whq, wlq = q(pool['xh']), q(pool['xl']), q(pool['th']), q(pool['tl'])
    mm = (lambda u, v: torch.einsum('pqk,fqk->qfp', u, v))            # [4, 512, P]
    acc0, acc1 = mm(xhq, whq), mm(xlq, whq) + mm(xhq, wlq)
    t0 = mm(xhq.abs(), whq.abs())
    t1 = mm(xlq.abs(), whq.abs()) + mm(xhq.abs(), wlq.abs())
    parts = acc0 + acc1 / LO
    hid = lrelu(parts.sum(0) + _t(b1)[:, None])                       # [512, P]
    out = (_t(w2) @ hid + _t(b2)[:, None]).t().contiguous()           # [P, 2]
    pool.update(acc0=acc0, acc1=acc1, t0=t0, t1=t1, parts=parts, hid=hid, out=out,
                lin2_abs=(_t(w2).abs() @ hid.abs() + _t(b2).abs()[:, None]).t())
    pool['true'] = pool['x64'] @ pool['w1_64'].t()                    # [P, 512]
    pool['true_abs'] = pool['x64'].abs() @ pool['w1_64'].abs().t()
    return pool


def stat_units(pool):
    """actor_exact_ref.stat_units on an x3 pool (the same fields)."""
    return R.stat_units(pool)


def out4_units(pool):
    return R.out4_units(pool)


def perturbed_tap(pool, co=9):
    """The pool's inputs with one weight tap of output channel co raised by one
    grain of its lo half (LO_GRAIN; the first tap whose hi half is not zero
    and whose lo half has room): the sensitivity test's expectation.  Returns
    (weights float32, v float64, the tap (ci, ky, kx))."""
    st = GEOM[pool['layer']][4]
    w = pool['w64'].clone()
    hi = torch.round(w[co])
    tap = tuple(((hi != 0) & (w[co] - hi <= 0)).nonzero()[0].tolist())
    w[(co,) + tap] += LO_GRAIN
    e, t32 = fold32(w.numpy(), pool['sc'].numpy())
    assert (e == pool['e'].numpy()).all()
    th, tl = split16(t32)
    nchw = (lambda q: q.permute(0, 3, 1, 2))
    acc0, acc1, _, _ = model3(nchw(pool['xh']), nchw(pool['xl']), _t(th), _t(tl), st)
    b2 = pool['b'].double()[None] + (w[None] * pool['sh'][:, None, :, None, None]).flatten(2).sum(-1)
    scale = torch.ldexp(torch.ones(P, dtype=torch.float64), pool['e'])[:, None, None, None]
    return w.float(), lrelu((acc0 + acc1 / LO) * scale + b2[:, :, None, None]), tap
