"""The train-mode BatchNorm tail (include/dttrain.h: dt_bn_leaky_fwd,
dt_bn_leaky_apply, dt_bn_leaky_bwd) through the C ABI at the edges of its
partition and on ill-conditioned channels, against a float64 restatement
written here (`tail_ref`), with per-channel bounds that have no floor.

The restatement starts from the kernel's own float32 activation
a32 = leaky(fl32(z + bias)) (one add, one compare, one multiply) and does
everything after that in float64; LeakyReLU's derivative takes its branch from
the sign of z + bias, an exact zero (either sign) the slope branch, as
torch.nn.functional.leaky_relu does.  `test_reference_matches_float64_autograd`
(CPU) checks it against float64 torch autograd to 1e-12.

Bounds, per channel c, with u = 2^-24 and cond_c = 1 + |mean_c| / sqrt(var_c + eps):
  y            |err| <= K_Y u cond_c |gamma_c|            per element
  dz           |err| <= K_G u cond_c S_c                  per element, S_c = max |dz64| of the channel
  dbias, dgamma, dbeta
               |err| <= K_G u cond_c T_c                  T_c = the sum of the absolute terms summed
  mean         |err| <= 4 u (|mean_c| + std_c);  running_mean: the same times momentum
  invstd, running_var   relative K_Y u cond_c
  a constant channel: y == beta exactly, invstd == fl32(1 / sqrt(eps)) within 1 ulp.
K_Y and K_G are 4 times the worst error, in those units, of CPU float32 torch
(F.batch_norm and autograd on a32) against `tail_ref` on the input family of
`family()` at m = 257, slopes {0.01, 0, 1, 0.2, -0.2} (`cpu_float32_units`;
the kernel's reduction order differs from torch's, the factor 4 is the room
that gets).  Measured, worst over channels and slopes:
  y 6.17 (the constant channel, whose mean torch does not get exactly; 1.89
  elsewhere), invstd 0.94, running_var 1.38             -> K_Y = 4 * 6.17 = 24.7
  dz 1.54 (a channel with cond 1.3: the three roundings of da itself; 0.05 or
  less, i.e. up to 21 u S_c, on the channels with cond > 100),
  dbias 0.21, dgamma 0.20, dbeta 0.11                   -> K_G = 4 * 1.54 = 6.2
Channels whose unit is zero (a constant channel's variance and dgamma) are
left out of that measurement, torch's float32 mean of a constant not being the
constant; the kernel is held to them (zero error on a zero unit).  At
m = 70001 torch's CPU float32 sums lose far more (y 1160, dz 44 of these
units), which would only loosen the bounds, so that size sets no constant.

Four places where the forms above cannot hold for any float32 kernel, and
what stands there instead (reasoned, not measured):
* m <= 3: dz is what the backward leaves of dy after taking two of its at
  most three degrees of freedom a channel away: identically zero at m = 2,
  and at m = 3 as small against its own terms as chance has it, so S_c says
  nothing about the roundings of those terms.  There S_c is the channel's
  largest, and T_c of dbias the sum, of the terms' sizes
  |gamma invstd| (|dy| + |dbeta / m| + |xhat dgamma / m|) (times |slope| on
  that branch).
* dgamma in the partition-edge test (`edges`): mean_invstd holds the mean in
  float32, so each xhat carries the mean's error times invstd, and dgamma
  that times sum(dy) = dbeta.  Over a few pixels of a channel whose variance
  is below eps (|xhat| << 1) nothing averages that away and it exceeds any
  multiple of T_c.  The mean's own allowed error carried through,
  4 u (|mean_c| + std_c) invstd_c |dbeta_c|, is added to dgamma's bound there.
  The ill-conditioned cases at m = 257 and 70001 keep the plain form.
* running_var in the partition-edge test: eps is not part of it, so what
  limits it is |mean_c| / std_c itself, the variance being made of
  differences from a float32 mean; cond_c, which has eps under its root, says
  less than that once the variance is below eps, as the variance of two or
  three pixels is whenever they happen to lie close.  There the relative bound
  is K_Y u (1 + |mean_c| / std_c).
* `updates` > 1, or running statistics that do not start at zero: a move
  (1 - momentum) r + momentum s is four float32 roundings of its own (the
  factor 1 - momentum, two products, the add), each at most u times
  max(|r0|, |s|).  The bound is the statistic's own bound times
  1 - (1 - momentum)^updates (which is `momentum` for one move) plus
  4 updates u max(|r0|, |s|).  With r0 = 0 and one move that extra term is
  not used: the plain bound stands.

The kernels' own worst figures in these units on an MI355X (printed by every
test before it asserts): y 7.3, mean 2.4 (4.02 at m = 127 and 3.6-3.8 at
65537 and 70001 before the statistics' last merge became a tree), invstd 0.94,
running_var 9.8, dz 2.1, dbias 0.61, dgamma 1.7, dbeta 0.60.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

C = 32
U = 2.0 ** -24
EPS = float(np.float32(1e-5))
MOM = float(np.float32(0.1))
K_Y = 24.7
K_G = 6.2
PARTS = 256 * C * 3          # floats of partials before the counters (dttrain.hip)
SLOPES = [0.01, 0.0, 1.0, 0.2, -0.2]


# ---- the float64 restatement --------------------------------------------------------------
def leaky32(z, bias, slope):
    """The kernel's float32 activation and the branch its derivative takes."""
    t = z + bias                                   # float32, one rounding
    s = torch.tensor(slope, dtype=torch.float32)
    pos = t > 0
    return torch.where(pos, t, t * s), pos


def tail_ref(z, bias, gamma, beta, slope, eps, momentum, updates, dy, rm0=None, rv0=None):
    """float32 CPU tensors z, dy [m, 32], bias, gamma, beta [32] -> a dict of
    float64 results (and the absolute-term sums the bounds use)."""
    m = z.shape[0]
    a32, pos = leaky32(z, bias, slope)
    s64 = float(np.float32(slope))
    a = a32.double()
    g, b, d = gamma.double(), beta.double(), dy.double()
    mean = a.mean(0)
    var = ((a - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (a - mean) * invstd
    y = xhat * g + b
    unbiased = var * m / (m - 1) if m > 1 else var
    rm = torch.zeros(C, dtype=torch.float64) if rm0 is None else rm0.double().clone()
    rv = torch.zeros(C, dtype=torch.float64) if rv0 is None else rv0.double().clone()
    for _ in range(updates):
        rm = (1.0 - momentum) * rm + momentum * mean
        rv = (1.0 - momentum) * rv + momentum * unbiased
    dbeta = d.sum(0)
    dgamma = (d * xhat).sum(0)
    da = g * invstd * (d - dbeta / m - xhat * dgamma / m)
    dz = torch.where(pos, da, s64 * da)
    terms = g.abs() * invstd * (d.abs() + dbeta.abs() / m + xhat.abs() * dgamma.abs() / m)
    terms = torch.where(pos, terms, abs(s64) * terms)
    return dict(a32=a32, gamma=g, y=y, mean=mean, var=var, invstd=invstd, unbiased=unbiased, rm=rm, rv=rv,
                dz=dz, dbias=dz.sum(0), dgamma=dgamma, dbeta=dbeta,
                t_dbias=dz.abs().sum(0), t_dgamma=(d * xhat).abs().sum(0), t_dbeta=d.abs().sum(0),
                cond=1.0 + mean.abs() / torch.sqrt(var + eps),
                cancel=terms.amax(0), cancel_sum=terms.sum(0))


def family(m, seed=0):
    """The input family of the module docstring (float32 CPU tensors):
    channel c's pre-activation has std 2^(-10 + c mod 17) around std 2^(c mod 11)
    (|mean| / std up to 2^10); channels 9 and 20 have negative offsets (wholly
    on the slope branch); channel 31 is constant; a tenth of channel 5's z is
    -bias (z + bias = +0) and a tenth of channel 6's, whose bias is -0.0, is
    zero, a few of them -0.0 (z + bias = -0.0); gamma in [0.5, 1.5); dy's
    channel c scaled by 2^(-2c)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    c = torch.arange(C)
    std = 2.0 ** (-10.0 + (c % 17).double())
    off = std * 2.0 ** (c % 11).double()
    off[9], off[20] = -off[9], -off[20]
    pre = off + std * torch.randn(m, C, generator=gen, dtype=torch.float64)
    bias = (std * (torch.rand(C, generator=gen, dtype=torch.float64) * 2 - 1)).float()
    bias[6] = -0.0
    z = (pre - bias.double()).float()
    z[:, 31] = 0.8125
    n0 = m // 10
    rows = torch.randperm(m, generator=gen)[:2 * n0]
    z[rows[:n0], 5] = -bias[5]
    z[rows[n0:], 6] = 0.0
    z[rows[n0:n0 + (n0 + 3) // 4], 6] = -0.0
    gamma = (0.5 + torch.rand(C, generator=gen)).float()
    beta = (torch.rand(C, generator=gen) - 0.5).float()
    dy = (torch.randn(m, C, generator=gen, dtype=torch.float64) * 2.0 ** (-2.0 * c.double())).float()
    return z, bias, gamma, beta, dy


@functools.lru_cache(maxsize=32)
def _case(m, slope, seed=0):
    """(inputs, reference) shared by the tests; never modified."""
    inp = family(m, seed)
    z, bias, gamma, beta, dy = inp
    return inp, tail_ref(z, bias, gamma, beta, slope, EPS, MOM, 1, dy)


SKIP_ZERO_UNITS = [False]      # cpu_float32_units only


def _units(err, unit):
    """The worst err / unit; inf where the unit is zero and the error is not."""
    inf = 0.0 if SKIP_ZERO_UNITS[0] else float('inf')
    r = torch.where(unit > 0, err / unit.clamp_min(1e-300),
                    torch.where(err > 0, torch.full_like(err, inf), torch.zeros_like(err)))
    return float(r.max())


def errors_in_units(m, ref, y, mean, invstd, rm, rv, dz, dbias, dgamma, dbeta, updates=1,
                    rm0=None, rv0=None, edges=False):
    """Each output's worst error in the units of its bound (module docstring)
    -> {name: (worst, allowed)}; float64 CPU tensors against tail_ref's."""
    cond = ref['cond']
    out = {}
    std = torch.sqrt(ref['var'])
    grow = 1.0 - (1.0 - MOM) ** updates
    moved = updates > 1 or rm0 is not None
    if y is not None:
        out['y'] = (_units((y - ref['y']).abs(), (U * cond * ref['gamma'].abs()).expand_as(y)), K_Y)
        out['mean'] = (_units((mean - ref['mean']).abs(), U * (ref['mean'].abs() + std)), 4.0)
        out['invstd'] = (_units((invstd - ref['invstd']).abs(), U * cond * ref['invstd']), K_Y)
        r0 = torch.zeros(C, dtype=torch.float64) if rm0 is None else rm0.double().abs()
        v0 = torch.zeros(C, dtype=torch.float64) if rv0 is None else rv0.double().abs()
        extra_m = 4 * updates * U * torch.maximum(r0, ref['mean'].abs()) * moved
        extra_v = 4 * updates * U * torch.maximum(v0, ref['unbiased']) * moved
        out['running_mean'] = (_units((rm - ref['rm']).abs(),
                                      U * (ref['mean'].abs() + std) * grow + extra_m / 4.0), 4.0)
        unit_v = U * cond * ref['unbiased']
        if edges:                        # (1 + |mean| / std) unbiased, finite at std = 0
            unit_v = U * (ref['unbiased'] + ref['mean'].abs() * std * m / max(m - 1, 1))
        out['running_var'] = (_units((rv - ref['rv']).abs(), unit_v * grow + extra_v / K_Y), K_Y)
    if dz is not None:
        s = ref['dz'].abs().amax(0)
        t = ref['t_dbias']
        if m <= 3:                       # dz far below its own terms: their sizes
            s, t = ref['cancel'], ref['cancel_sum']
        out['dz'] = (_units((dz - ref['dz']).abs(), (U * cond * s).expand_as(dz)), K_G)
        out['dbias'] = (_units((dbias - ref['dbias']).abs(), U * cond * t), K_G)
        carried = 4 * U * (ref['mean'].abs() + std) * ref['invstd'] * ref['dbeta'].abs() * edges
        out['dgamma'] = (_units((dgamma - ref['dgamma']).abs(),
                                U * cond * ref['t_dgamma'] + carried / K_G), K_G)
        out['dbeta'] = (_units((dbeta - ref['dbeta']).abs(), U * cond * ref['t_dbeta']), K_G)
    return out


def _assert_within(errs, what):
    print(what, ' '.join('%s %.3g/%.3g' % (k, v[0], v[1]) for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, '%s: worst error in units of the bound / allowed: %s' % (what, bad)


# ---- CPU: the restatement itself, and where K_Y / K_G come from ---------------------------
@pytest.mark.parametrize('slope', [0.01, 0.0, -0.2])
def test_reference_matches_float64_autograd(slope):
    """tail_ref against float64 torch autograd of
    F.batch_norm(F.leaky_relu(z + b, slope), ..., training=True), 1e-12 relative
    (to each channel's largest element; sums to the sum of their absolute
    terms).  The float64 graph's activation differs from a32 by a32's own
    float32 rounding of the product with the slope; that difference is added
    back as a constant, which no derivative sees, so both sides start from the
    same values."""
    torch.manual_seed(5)
    m = 300
    z = torch.randn(m, C) * 2 + 0.3
    z[:7, 3] = 0.0
    z[3:7, 3] = -0.0
    bias = torch.randn(C) * 0.5
    bias[3] = 0.0                                   # channel 3: exact zeros
    gamma, beta = torch.rand(C) + 0.5, torch.rand(C) - 0.5
    dy = torch.randn(m, C)
    rm0, rv0 = torch.randn(C), torch.rand(C) + 0.5
    ref = tail_ref(z, bias, gamma, beta, slope, EPS, MOM, 3, dy, rm0, rv0)
    s64 = float(np.float32(slope))
    zz, bb = z.double().requires_grad_(True), bias.double().requires_grad_(True)
    gg, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    for _ in range(3):
        act = F.leaky_relu(zz + bb, s64)
        act = act + (ref['a32'].double() - act).detach()
        y = F.batch_norm(act, rm, rv, gg, be, True, MOM, EPS)
    y.backward(dy.double())
    a = ref['a32'].double()

    def close(got, want, scale):
        assert float(((got - want).abs() / scale).max()) <= 1e-12
    close(ref['y'], y.detach(), y.detach().abs().amax(0))
    close(ref['mean'], a.mean(0), a.abs().amax(0))
    close(ref['invstd'], 1.0 / torch.sqrt(a.var(0, unbiased=False) + EPS), ref['invstd'])
    close(ref['rm'], rm, rm.abs() + a.abs().amax(0))
    close(ref['rv'], rv, rv.abs())
    close(ref['dz'], zz.grad, zz.grad.abs().amax(0))
    close(ref['dbias'], bb.grad, ref['t_dbias'])
    close(ref['dgamma'], gg.grad, ref['t_dgamma'])
    close(ref['dbeta'], be.grad, ref['t_dbeta'])
    # an exact zero of either sign takes the slope branch
    assert not leaky32(z, bias, slope)[1][:7, 3].any()


def cpu_float32_units(m, slope):
    """CPU float32 torch (F.batch_norm and autograd on a32) on family(m) in the
    units of the bounds: what K_Y and K_G are four times the worst of."""
    (z, bias, gamma, beta, dy), ref = _case(m, slope)
    a32 = ref['a32'].clone().requires_grad_(True)
    g32, b32 = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = torch.zeros(C), torch.zeros(C)
    y = F.batch_norm(a32, rm, rv, g32, b32, True, MOM, EPS)
    y.backward(dy)
    _, pos = leaky32(z, bias, slope)
    dz = torch.where(pos, a32.grad, a32.grad * torch.tensor(slope, dtype=torch.float32))
    mean = ref['a32'].mean(0)
    invstd = 1.0 / torch.sqrt(ref['a32'].var(0, unbiased=False) + torch.tensor(EPS))
    d = (lambda t: t.detach().double())
    SKIP_ZERO_UNITS[0] = True
    try:
        return errors_in_units(m, ref, d(y), d(mean), d(invstd), d(rm), d(rv),
                               d(dz), d(dz.sum(0)), d(g32.grad), d(b32.grad))
    finally:
        SKIP_ZERO_UNITS[0] = False


def test_bound_constants_are_four_times_cpu_float32():
    """K_Y and K_G leave CPU float32 torch at least a factor 2 at m = 257 (the
    module docstring has the figures; a factor 2, not 4, so that another
    build of torch summing in another order does not fail this)."""
    for slope in SLOPES:
        e = cpu_float32_units(257, slope)
        print(slope, {k: round(v[0], 4) for k, v in e.items()})
        assert max(e[k][0] for k in ('y', 'invstd', 'running_var')) <= K_Y / 2
        assert max(e[k][0] for k in ('dz', 'dbias', 'dgamma', 'dbeta')) <= K_G / 2


# ---- GPU ----------------------------------------------------------------------------------
def _lib():
    from aido1_amd import _lib as lib_mod
    return lib_mod.lib()


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _new_work(dev):
    return torch.zeros(int(_lib().dt_train_work_floats(0)), device=dev)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _fwd(dev, inp, slope, work, guard=None, updates=1, rm=None, rv=None, nbt=None, a=None):
    z, bias, gamma, beta = inp[:4]
    m = z.shape[0]
    rm = torch.zeros(C, device=dev) if rm is None else rm
    rv = torch.zeros(C, device=dev) if rv is None else rv
    y = torch.full_like(z, float('nan'))
    mi = torch.full((2 * C,), float('nan'), device=dev)
    rc = _lib().dt_bn_leaky_fwd(m, z.data_ptr(), bias.data_ptr(), slope, gamma.data_ptr(),
                                beta.data_ptr(), EPS, MOM, rm.data_ptr(), rv.data_ptr(), _ptr(nbt),
                                updates, _ptr(a), y.data_ptr(), mi.data_ptr(), work.data_ptr(),
                                guard.ptr() if guard is not None else None, _stream(dev))
    assert rc == 0
    return y, mi, rm, rv


def _bwd(dev, inp, mi, slope, work, guard=None, dy=None):
    z, bias, gamma = inp[:3]
    dy = inp[4] if dy is None else dy
    dz = torch.full_like(z, float('nan'))
    g = torch.full((3, C), float('nan'), device=dev)      # dbias, dgamma, dbeta
    rc = _lib().dt_bn_leaky_bwd(z.shape[0], dy.data_ptr(), z.data_ptr(), bias.data_ptr(),
                                mi.data_ptr(), gamma.data_ptr(), slope, dz.data_ptr(),
                                g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), work.data_ptr(),
                                guard.ptr() if guard is not None else None, _stream(dev))
    assert rc == 0
    return dz, g


def _scratch_is_clean(work, fwd):
    counters = work.view(torch.int32)[PARTS:PARTS + 3]
    assert counters.tolist() == [0, 0, 0]
    if fwd:
        assert not work[:PARTS].view(256, C, 3)[:, :, 0].any()


def _check(m, ref, fwd=None, bwd=None, what='', **kw):
    d = (lambda t: t.double().cpu())
    y = mean = invstd = rm = rv = dz = dbias = dgamma = dbeta = None
    if fwd is not None:
        y, mean, invstd, rm, rv = d(fwd[0]), d(fwd[1][:C]), d(fwd[1][C:]), d(fwd[2]), d(fwd[3])
    if bwd is not None:
        dz, dbias, dgamma, dbeta = d(bwd[0]), d(bwd[1][0]), d(bwd[1][1]), d(bwd[1][2])
    _assert_within(errors_in_units(m, ref, y, mean, invstd, rm, rv, dz, dbias,
                                   dgamma, dbeta, **kw), what)


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# large and small grids in turn: 256, 1, 256, 1, 256, 1, 256, 1, 255, 1, 3, 2, 2, 1, 2, 1
EDGE_MS = [280896, 1, 70001, 2, 65537, 3, 65281, 127, 65280, 128, 513, 129, 511, 255, 257, 256]


@pytest.mark.gpu
def test_partition_edges_share_one_scratch(gpu):
    """Forward and backward at every m where grid_of or a thread's item count
    changes, in an order that alternates large and small grids, on ONE forward
    and ONE backward scratch zeroed once: outputs within the bounds, the guard
    (lost partial, non-finite) silent, counters and partial counts left at
    zero, a second launch and a launch on fresh scratch bit-identical."""
    from aido1_amd.guard import Guard
    slope = 0.01
    guard = Guard(gpu)
    wf, wb = _new_work(gpu), _new_work(gpu)
    for m in EDGE_MS:
        if m > 100000:
            inp = family(m)
            ref = tail_ref(*inp[:4], slope, EPS, MOM, 1, inp[4])
        else:
            inp, ref = _case(m, slope)
        dev = [t.to(gpu) for t in inp]
        f1 = _fwd(gpu, dev, slope, wf, guard)
        _scratch_is_clean(wf, True)
        b1 = _bwd(gpu, dev, f1[1], slope, wb, guard)
        _scratch_is_clean(wb, False)
        _check(m, ref, f1, b1, 'm=%d' % m, edges=True)
        f2 = _fwd(gpu, dev, slope, wf, guard)
        _scratch_is_clean(wf, True)
        b2 = _bwd(gpu, dev, f2[1], slope, wb, guard)
        _scratch_is_clean(wb, False)
        f3 = _fwd(gpu, dev, slope, _new_work(gpu), guard)
        b3 = _bwd(gpu, dev, f3[1], slope, _new_work(gpu), guard)
        for f, b in ((f2, b2), (f3, b3)):
            assert _same_bits(f1[:2], f[:2]), m
            assert _same_bits((b1[0], b1[1]), (b[0], b[1])), m
        assert guard.read()['stages'] == [], m
        if m == 1:
            assert torch.equal(f1[0], dev[3].expand(1, C))
            assert torch.isfinite(f1[1]).all()


@pytest.mark.gpu
@pytest.mark.parametrize('slope', SLOPES)
@pytest.mark.parametrize('m', [257, 70001])
def test_ill_conditioned_channels(gpu, m, slope):
    """The family of the module docstring at every slope (1: a plain
    BatchNorm; -0.2: the activation's sign is not the pre-activation's):
    per-channel bounds, the constant channel exact."""
    inp, ref = _case(m, slope)
    dev = [t.to(gpu) for t in inp]
    f = _fwd(gpu, dev, slope, _new_work(gpu))
    b = _bwd(gpu, dev, f[1], slope, _new_work(gpu))
    _check(m, ref, f, b, 'm=%d slope=%g' % (m, slope))
    const = [31] + ([9, 20] if slope == 0.0 else [])     # a == 0 on a wholly negative channel
    for c in const:
        assert torch.equal(f[0][:, c], dev[3][c].expand(m)), c
    want = np.float32(1.0) / np.sqrt(np.float32(EPS))
    got = f[1][C + 31].cpu().numpy()
    assert abs(float(got) - float(want)) <= float(np.spacing(want))


@pytest.mark.gpu
@pytest.mark.parametrize('m', [257, 70001])
def test_derivative_branch_unmoved_for_positive_slope(gpu, m):
    """For slope >= 0 the sign of z + bias and the activation's agree on every
    input, exact zeros included: dz and dbias' terms equal, bit for bit, the
    kernel's float32 formula with the branch taken from the ACTIVATION (how it
    was taken before), restated on the CPU from the kernel's mean_invstd,
    dgamma and dbeta."""
    slope = 0.01
    inp, ref = _case(m, slope)
    z, bias, gamma, beta, dy = inp
    dev = [t.to(gpu) for t in inp]
    f = _fwd(gpu, dev, slope, _new_work(gpu))
    dz, g = _bwd(gpu, dev, f[1], slope, _new_work(gpu))
    mi, g = f[1].cpu(), g.cpu()
    x = ref['a32']
    inv_m = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(m), dtype=torch.float32)
    mu, inv = mi[:C], mi[C:]
    k1, k2, k3 = gamma * inv, g[2] * inv_m, g[1] * inv_m
    xh = (x - mu) * inv
    t = xh * k3
    da = k1 * ((dy - k2) - t)
    old = torch.where(x > 0, da, da * torch.tensor(slope, dtype=torch.float32))
    assert torch.equal(dz.cpu().view(torch.int32), old.view(torch.int32))
    assert np.array_equal(g[0].numpy(), _sum_in_kernel_order(old.numpy()))


def _sum_in_kernel_order(v):
    """The per-channel float32 sum of v [m, 32] in dttrain.hip's order: a
    thread's pixels (grid steps of 128 a workgroup), 4 slots of the workgroup
    32 apart, those 32 sums, then the workgroups 32 apart and those 32 sums."""
    m = v.shape[0]
    grid = min(256, max(1, (m * 8 + 2047) // 2048))
    steps = (m + grid * 128 - 1) // (grid * 128)
    pad = np.zeros((steps * grid * 128, C), np.float32)
    pad[:m] = v

    def chain(x):                       # sequential float32 sum over axis 0
        t = np.zeros(x.shape[1:], np.float32)
        for row in x:
            t = t + row
        return t
    acc = chain(pad.reshape(steps, grid, 128, C))                # [grid, slot, C]
    red2 = chain(acc.reshape(grid, 4, 32, C).transpose(1, 0, 2, 3))   # [grid, 32, C]
    part = np.zeros((256, C), np.float32)
    part[:grid] = chain(red2.transpose(1, 0, 2))
    return chain(chain(part.reshape(8, 32, C)))


@pytest.mark.gpu
@pytest.mark.parametrize('slope', [0.01, -0.2])
@pytest.mark.parametrize('m', [257, 70001])
def test_backward_is_homogeneous_in_dy(gpu, m, slope):
    """Every operation of both backward kernels is linear in dy: dy * 2^-20
    gives dz, dbias, dgamma and dbeta times 2^-20, bit for bit."""
    inp, _ = _case(m, slope)
    dev = [t.to(gpu) for t in inp]
    f = _fwd(gpu, dev, slope, _new_work(gpu))
    work = _new_work(gpu)
    dz, g = _bwd(gpu, dev, f[1], slope, work)
    k = 2.0 ** -20
    dz2, g2 = _bwd(gpu, dev, f[1], slope, work, dy=dev[4] * k)
    assert torch.isfinite(dz2).all() and (dz2 != 0).sum() == (dz != 0).sum()
    assert _same_bits((dz * k, g * k), (dz2, g2))


@pytest.mark.gpu
@pytest.mark.parametrize('slope', [0.01, -0.2])
@pytest.mark.parametrize('m', [257, 70001])
def test_activation_output_and_apply(gpu, m, slope):
    """With `a` asked for it is torch's float32 leaky_relu(z + bias) bit for
    bit and nothing else moves; dt_bn_leaky_apply on the forward's
    mean_invstd writes the forward's y."""
    inp, _ = _case(m, slope)
    dev = [t.to(gpu) for t in inp]
    z, bias, gamma, beta = dev[:4]
    f0 = _fwd(gpu, dev, slope, _new_work(gpu))
    a = torch.full_like(z, float('nan'))
    f1 = _fwd(gpu, dev, slope, _new_work(gpu), a=a)
    assert _same_bits(f0, f1)
    want = F.leaky_relu(inp[0] + inp[1], slope)
    assert torch.equal(a.cpu().view(torch.int32), want.view(torch.int32))
    y = torch.full_like(z, float('nan'))
    rc = _lib().dt_bn_leaky_apply(m, z.data_ptr(), bias.data_ptr(), slope, f0[1].data_ptr(),
                                  gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _stream(gpu))
    assert rc == 0
    assert _same_bits((y,), (f0[0],))


@pytest.mark.gpu
@pytest.mark.parametrize('m', [257, 70001])
def test_repeated_running_updates(gpu, m):
    """`updates` in {1, 2, 5}, with and without num_batches_tracked, from
    running statistics that are not zero: y and mean_invstd do not depend on
    it, the running statistics follow the float64 loop, the counter moves by
    `updates`."""
    slope = 0.01
    inp, _ = _case(m, slope)
    dev = [t.to(gpu) for t in inp]
    gen = torch.Generator().manual_seed(m)
    rm0 = torch.randn(C, generator=gen)
    rv0 = torch.rand(C, generator=gen) * 1.5 + 0.5
    first = None
    for updates in (1, 2, 5):
        ref = tail_ref(*inp[:4], slope, EPS, MOM, updates, inp[4], rm0, rv0)
        for counted in (True, False):
            nbt = torch.tensor([7], dtype=torch.int64, device=gpu) if counted else None
            f = _fwd(gpu, dev, slope, _new_work(gpu), updates=updates, rm=rm0.to(gpu),
                     rv=rv0.to(gpu), nbt=nbt)
            first = first or f
            assert _same_bits(first[:2], f[:2])
            _check(m, ref, f, None, 'm=%d updates=%d' % (m, updates), updates=updates,
                   rm0=rm0, rv0=rv0)
            if counted:
                assert int(nbt) == 7 + updates


# ---- Adam and the soft update at the chunk edges (DT_MT_CHUNK = 4096) ---------------------
MT_SIZES = [1, 255, 256, 4095, 4096, 4097, 8192, 12289]
SENTINEL = 12345.0


def _carve(dev, sizes, fill):
    """One tensor per size out of a single storage, a sentinel after each;
    fill(n) gives a tensor's content.  -> (views, the storage, sentinel mask)."""
    buf = torch.full((sum(sizes) + len(sizes),), SENTINEL, device=dev)
    mask = torch.ones_like(buf, dtype=torch.bool)
    views, at = [], 0
    for n in sizes:
        buf[at:at + n] = fill(n)
        mask[at:at + n] = False
        views.append(buf[at:at + n])
        at += n + 1
    return views, buf, mask


@pytest.mark.gpu
def test_adam_at_chunk_edges(gpu):
    """One DeviceAdam over flat parameters of 1 ... 12289 elements (one
    workgroup a chunk of 4096, partial and exact last chunks), three steps
    with a changing lr against torch.optim.Adam; the element after each
    parameter's, gradient's and moment's storage is not written."""
    from aido1_amd.optim import DeviceAdam
    torch.manual_seed(21)
    pv, pbuf, pmask = _carve(gpu, MT_SIZES, lambda n: torch.randn(n, device=gpu))
    gv, gbuf, gmask = _carve(gpu, MT_SIZES, lambda n: torch.zeros(n, device=gpu))
    mv, mbuf, mmask = _carve(gpu, MT_SIZES, lambda n: torch.zeros(n, device=gpu))
    vv, vbuf, vmask = _carve(gpu, MT_SIZES, lambda n: torch.zeros(n, device=gpu))
    params = [torch.nn.Parameter(v) for v in pv]
    ref = [torch.nn.Parameter(v.detach().clone()) for v in pv]
    opt = DeviceAdam(params, gpu)
    for p, g, m1, m2 in zip(params, gv, mv, vv):
        p.grad = g
        opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq'] = m1, m2
    ropt = torch.optim.Adam(ref, lr=0.0)
    for k in range(3):
        lr = 1e-3 * (1.0 - 0.1 * k)
        opt.param_groups[0]['lr'].fill_(lr)
        ropt.param_groups[0]['lr'] = lr
        for p, q in zip(params, ref):
            g = torch.randn_like(p) * (0.1 + k)
            p.grad.copy_(g)
            q.grad = g.clone()
        opt.step()
        ropt.step()
    assert opt._table is not None and opt._table.n_chunks == 1 + 1 + 1 + 1 + 1 + 2 + 2 + 4
    for p, q in zip(params, ref):
        torch.testing.assert_close(p, q, rtol=1e-6, atol=1e-7)
        st, rst = opt.state[p], ropt.state[q]
        torch.testing.assert_close(st['exp_avg'], rst['exp_avg'], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(st['exp_avg_sq'], rst['exp_avg_sq'], rtol=1e-6, atol=1e-10)
        assert float(st['step']) == 3.0
    assert int(opt._counter) == 0
    for buf, mask in ((pbuf, pmask), (gbuf, gmask), (mbuf, mmask), (vbuf, vmask)):
        assert bool((buf[mask] == SENTINEL).all())


@pytest.mark.gpu
def test_soft_update_at_chunk_edges(gpu):
    """dt_soft_update over the same sizes = torch's t * (1 - tau) + p * tau bit
    for bit, the element after each target's storage not written."""
    from aido1_amd.trainer import soft_update
    torch.manual_seed(22)

    class Flat(torch.nn.Module):
        def __init__(self, views):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(v) for v in views])
    tv, tbuf, tmask = _carve(gpu, MT_SIZES, lambda n: torch.randn(n, device=gpu))
    sv, sbuf, smask = _carve(gpu, MT_SIZES, lambda n: torch.randn(n, device=gpu))
    a, b = Flat(tv), Flat(sv)
    src = sbuf.clone()
    tau = 0.005
    expect = [t.data * (1.0 - tau) + s.data * tau for t, s in zip(a.parameters(), b.parameters())]
    soft_update(a, b, tau)
    for t, e in zip(a.parameters(), expect):
        assert torch.equal(t.data, e)
    assert bool((tbuf[tmask] == SENTINEL).all()) and torch.equal(sbuf, src)
