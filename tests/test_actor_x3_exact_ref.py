"""The conditions under which tests/test_gpu_actor_x3_exact.py may demand bit
equality of the x3 actor kernels, asserted on every pool it uses
(tests/actor_x3_exact_ref.py): representability of every operand as hi + 2^-11
lo, the bit widths of the worst partial sums of both accumulators, of bias'
and of lin2, the shares of lo != 0, the degenerate and the rare-branch
channels, the distance of the three-product model from the true convolution,
and the constants of the tolerances that remain.  These are caps, not
measurements: a pool that breaks one of them makes the GPU equality
meaningless."""
import numpy as np
import pytest
import torch

import actor_exact_ref as R
import actor_x3_exact_ref as X

POOLS32 = [(layer, seed, var) for layer in (2, 3, 4) for seed, var in X.VARIANTS32X]
IDS32 = ['conv%d-set%d-%s' % p for p in POOLS32]
LIMIT = 2.0 ** 24
FP16_MIN_NORMAL = 2.0 ** -14


def _f32_exact(t):
    return bool((t.float().double() == t).all())


def _f16_exact(t):
    return bool((t.half().double() == t).all())


def _sum_exact(terms_abs, g):
    """Sums whose terms are multiples of g and whose magnitudes add up to less
    than 2^24 g: every partial sum in any order is a float32 number."""
    return np.isfinite(g) and float(terms_abs) < LIMIT * g


def _operand_grains(pool, i):
    """Sample i's finest product of each accumulator, by input channel (the
    folded weights and, in the sublo variant, the inputs scale by channel)."""
    xh, xl, th, tl = (pool[k] for k in ('xh', 'xl', 'th', 'tl'))
    cdim = xh.shape[1] if pool['layer'] == 1 else xh.shape[-1]
    g0 = g1 = np.inf
    for c in range(cdim):
        xs = (lambda q: q[i, c] if pool['layer'] == 1 else q[i, ..., c])
        ws = (lambda q: q[i if q.shape[0] > 1 else 0, :, c])
        g0 = min(g0, X.grain(xs(xh)) * X.grain(ws(th)))
        g1 = min(g1, X.grain(xs(xl)) * X.grain(ws(th)), X.grain(xs(xh)) * X.grain(ws(tl)))
    return g0, g1


def _check_model(pool):
    """What every convolution pool must keep (module docstring)."""
    x, xh, xl = pool['x'], pool['xh'], pool['xl']
    assert _f32_exact(x) and _f16_exact(xh) and _f16_exact(xl)
    assert torch.equal(xh + xl / X.LO, x)                       # the pair is the operand
    th, tl = pool['th'], pool['tl']
    assert torch.isfinite(th).all() and torch.isfinite(tl).all()
    assert _f16_exact(th) and _f16_exact(tl)
    for i in range(X.P):
        g0, g1 = _operand_grains(pool, i)
        assert _sum_exact(pool['t0'][i].max(), g0), (i, 'acc0')
        assert _sum_exact(pool['t1'][i].max(), g1), (i, 'acc1')
    # the combination, the rescaled and biased value and LeakyReLU's product
    for key in ('acc0', 'acc1', 'comb', 'pre', 'v', 'c'):
        assert _f32_exact(pool[key]), key
    assert torch.equal(pool['v'], R.lrelu(pool['pre']))
    assert _f32_exact(pool['pre'] * R.SLOPE)
    neg, pos = (pool['pre'] < 0).double().mean().item(), (pool['pre'] > 0).double().mean().item()
    assert neg >= 0.25 and pos >= 0.25, (neg, pos)
    # both cross products decide bits: lo != 0 in a good share of both operands
    assert (xl != 0).double().mean().item() >= 0.35
    nz = th != 0
    assert (tl[nz] != 0).double().mean().item() >= 0.5
    # the dropped al bl 2^-22: not zero, and under 2^-22 sum |a||b|
    scale = 2.0 ** pool['e'].double()[:, None, None, None] if 'e' in pool else 1.0
    drop = (pool['comb'] - pool['true']) * scale
    assert drop.abs().max().item() > 0
    assert bool((drop.abs() <= 2.0 ** -22 * pool['true_abs'] * scale).all())
    # the store's split is exercised: the stored value needs its lo half
    if pool['layer'] != 4:
        d32 = pool['d32']
        assert (d32.half().float() != d32).double().mean().item() >= 0.5
    # distinct samples: a gather by the wrong index cannot pass
    for i in range(X.P):
        for j in range(i):
            assert not torch.equal(pool['v'][i], pool['v'][j])


@pytest.mark.parametrize('layer,seed,var', POOLS32, ids=IDS32)
def test_conv32x_pools_keep_the_three_product_model_exact(layer, seed, var):
    from aido1_amd.actor import hlb_decode
    pool = X.pool32x(layer, seed, var)
    ih, iw, _, _, st, _ = X.GEOM[layer]
    _check_model(pool)
    assert torch.equal(hlb_decode(pool['xin'], ih, iw, st), pool['x'])
    assert torch.equal(X.hlb_image(pool['x'].float(), st, 0), pool['xin'].view(torch.int16))
    # the folded weights: w sc 2^-e itself, as a pair; more than 11 significant bits
    flat = [X.FLAT_CI] if var == 'eps' else []
    keep = [c for c in range(32) if c not in flat]
    w, sc, e = pool['w64'], pool['sc'], pool['e'].double()
    exact = w[None] * sc[:, None, :, None, None] * (2.0 ** -e)[:, None, None, None, None]
    assert torch.equal(exact[:, :, keep], pool['t32'][:, :, keep])
    assert torch.equal((pool['th'] + pool['tl'] / X.LO)[:, :, keep], pool['t32'][:, :, keep])
    t = pool['t32'][:, :, keep]
    wide = [abs(v) / X.grain([v]) >= 2 ** 11 for v in t[t != 0][:4096].tolist()]
    assert np.mean(wide) >= 0.5
    # bias' = bias + sum w sh in any order
    bt = pool['bterms']
    gb = min(X.grain(bt), X.grain(pool['b']))
    assert _sum_exact((bt.abs().sum(-1) + pool['b'].double().abs()).max(), gb)
    assert _f32_exact(pool['b2'])
    assert X.grain(pool['sh']) >= 0.25 or var == 'eps'
    # the variant's branch is the one the pool takes
    want_e = {'rescale': [0 if i == X.RS_OFF else 2 for i in range(X.P)]}.get(var)
    if want_e:
        assert pool['e'].tolist() == want_e
        assert pool['gamma'][X.RS_CI] == 2.0 ** 16 and pool['beta'][X.RS_CI] != 0
        assert (pool['w'][:, X.RS_CI].abs().max() == 2.0 ** -12)
    elif var == 'sublo':
        assert pool['e'].min() >= 1 and pool['e'].max() == 3
        sub = (pool['xl'] != 0) & (pool['xl'].abs() < FP16_MIN_NORMAL)
        assert sub.double().mean().item() >= 0.1
        assert torch.equal(pool['v'], X.pool32x(layer, seed, 'plain')['v'])
    else:
        assert (pool['e'] == 0).all()
    if var == 'subw':
        t = pool['th'][:, :, X.SW_CI]
        rows = [co for co in range(32) if co not in X.ZERO_CO]
        assert bool((t[:, rows].abs() == 2.0 ** -16).all())     # an fp16 subnormal, in every tap
    else:
        nz = pool['th'] != 0
        assert bool((pool['th'][nz].abs() >= FP16_MIN_NORMAL).all())
    if var != 'sublo':
        nz = pool['xl'] != 0
        assert bool((pool['xl'][nz].abs() >= FP16_MIN_NORMAL).all())
    lo = pool['tl'][:, :, keep]
    assert bool((lo[lo != 0].abs() >= FP16_MIN_NORMAL).all())
    assert pool['th'].abs().max().item() <= 2.0 ** 15


@pytest.mark.parametrize('seed', [0, 1])
def test_conv1x_pools_keep_the_three_product_model_exact(seed):
    pool = X.pool1x(seed)
    _check_model(pool)
    fr = pool['x']
    assert fr.min().item() >= 0 and fr.max().item() <= 1
    assert torch.equal(pool['th'][0] + pool['tl'][0] / X.LO, pool['w64'])
    assert torch.equal(pool['frames'].double(), fr)


@pytest.mark.parametrize('layer', [2, 3, 4])
def test_flat_channel_contributes_exactly_beta(layer):
    """The eps variant's FLAT_CI under the fold: sc = gamma / sqrt(eps) is not
    dyadic and the folded weights are rounded, the inputs' halves are zero and
    sh is beta itself, so bias' holds exactly sum w beta for it; its weights
    are non-zero in every tap of every output channel that has weights."""
    pool = X.pool32x(layer, 0, 'eps')
    ci = X.FLAT_CI
    sc = pool['sc'][:, ci].numpy()
    assert not (np.frexp(sc)[0] == 0.5).any()
    others = np.delete(pool['sc'].numpy(), ci, 1)
    assert (np.frexp(others)[0] == 0.5).all()
    assert (pool['prev'][:, ci, :2] == 0).all()
    assert (pool['xh'][..., ci] == 0).all() and (pool['xl'][..., ci] == 0).all()
    beta = pool['beta'][ci].double()
    assert beta != 0 and (pool['sh'][:, ci] == beta).all()
    rows = [co for co in range(32) if co not in X.ZERO_CO]
    assert (pool['w'][rows, ci] != 0).all()
    exact = pool['w64'][None, :, ci] * pool['sc'][:, None, ci, None, None]
    assert not torch.equal(exact, pool['t32'][:, :, ci])         # the fold rounds here
    assert torch.isfinite(pool['th'][:, :, ci]).all()


@pytest.mark.parametrize('layer', [1, 2, 3, 4])
def test_degenerate_output_channels_are_in_the_x3_pools(layer):
    pools = [X.pool1x(0), X.pool1x(1)] if layer == 1 else [X.pool32x(layer, s, v)
                                                           for s, v in X.VARIANTS32X]
    for pool in pools:
        for co, sign in zip(X.ZERO_CO, (1, -1)):
            assert (pool['w'][co] == 0).all() and pool['b'][co].item() * sign > 0
            want_c = R.lrelu(pool['b'][co].double())
            assert (pool['c'][:, co] == want_c).all() and (pool['d'][:, co] == 0).all()
            if layer != 4:
                part = pool['part'][:, co]
                assert (part[:, :2] == 0).all() and (part[:, 2] == want_c).all()
                assert (pool['mean32'][:, co] == 0).all() and (pool['m2_32'][:, co] == 0).all()
            else:
                ob = pool['ob'][co]
                assert ob.item() * sign > 0
                assert (pool['want'].view(X.P, 32, -1)[:, co] == ob.double()).all()
                assert (pool['out32'].view(X.P, 32, -1)[:, co] == ob.double()).all()


def test_x3_bound_constants_are_four_times_cpu_float32():
    """K_STAT and K_OUT4 are four times the float32 restatements' worst error
    against float64 on the pools the GPU tests use (the helper's docstring has
    the figures), rounded up by less than a tenth."""
    worst = {1: [0.0, 0.0], 2: [0.0, 0.0], 3: [0.0, 0.0]}
    pools = [X.pool1x(0), X.pool1x(1)] + [X.pool32x(layer, s, v) for layer in (2, 3)
                                          for s, v in X.VARIANTS32X]
    for pool in pools:
        e = X.stat_units(pool)
        worst[pool['layer']] = [max(a, b) for a, b in zip(worst[pool['layer']], e)]
    print(worst)
    for layer, w in worst.items():
        for k, e in zip(X.K_STAT[layer], w):
            assert 4 * e <= k <= 4 * e + 0.1, (layer, k, e)
    e4 = max(X.out4_units(X.pool32x(4, s, v)) for s, v in X.VARIANTS32X)
    print(4, e4)
    assert 4 * e4 <= X.K_OUT4 <= 4 * e4 + 0.1, e4


@pytest.mark.parametrize('seed', [0, 1])
def test_head_pools_keep_lin1_and_lin2_exact(seed):
    pool = X.pool_head(seed)
    x, w1 = pool['x64'], pool['w1_64']
    assert _f32_exact(x) and _f32_exact(w1)
    assert torch.equal(pool['xh'] + pool['xl'] / X.LO, x)
    assert torch.equal(pool['th'] + pool['tl'] / X.LO, w1)
    assert (pool['xl'] != 0).double().mean().item() >= 0.35
    assert (pool['tl'][pool['th'] != 0] != 0).double().mean().item() >= 0.5
    # the 4032-term sums: each K quarter's two accumulators in any order
    g0 = X.grain(pool['xh']) * X.grain(pool['th'])
    g1 = min(X.grain(pool['xl']) * X.grain(pool['th']), X.grain(pool['xh']) * X.grain(pool['tl']))
    assert _sum_exact(pool['t0'].sum(0).max(), g0) and _sum_exact(pool['t1'].sum(0).max(), g1)
    assert _f32_exact(pool['acc0']) and _f32_exact(pool['acc1']) and _f32_exact(pool['parts'])
    # the K split's combination with b1, LeakyReLU, lin2's 512-term sums
    gp = min(X.grain(pool['parts']), X.grain(pool['b1']))
    assert _sum_exact((pool['parts'].abs().sum(0) + pool['b1'].double().abs()[:, None]).max(), gp)
    assert _f32_exact(pool['hid'])
    gh = min(X.grain(pool['hid']), X.grain(pool['b2']))
    assert _sum_exact(pool['lin2_abs'].max(), gh)
    assert _f32_exact(pool['out'])
    assert (pool['w2'] != 0).sum(1).tolist() == [X.W2_TAPS, X.W2_TAPS]
    hid = pool['hid']
    assert (hid < 0).double().mean().item() >= 0.25 and (hid > 0).double().mean().item() >= 0.25
    drop = (pool['parts'].sum(0).t() - pool['true']).abs()
    assert drop.max().item() > 0 and bool((drop <= 2.0 ** -22 * pool['true_abs']).all())
    for i in range(X.P):
        for j in range(i):
            assert not torch.equal(pool['out'][i], pool['out'][j])


@pytest.mark.parametrize('layer', [2, 3, 4])
def test_one_lo_grain_of_one_tap_changes_stored_bits_in_its_channel_only(layer):
    """The sensitivity test's perturbation (one tap raised by one grain of its
    lo half, 2^-13) is far under the 1e-5 max(1, max |ref|) of
    test_conv32x_layers_match_float64 and still changes the expectation, in
    channel co alone; the perturbed problem stays exact."""
    pool = X.pool32x(layer, 0, 'plain')
    co = 9
    _, v, _ = X.perturbed_tap(pool, co=co)
    ref = pool['v']
    err = (v - ref).abs()
    assert 0 < err.max().item() < 1e-5 * max(1.0, ref.abs().max().item())
    assert _f32_exact(v)
    diff = v != ref
    assert diff[:, co].any()
    diff[:, co] = False
    assert not diff.any()


def test_a_grid_a_bit_too_wide_is_refused():
    """The checks bite: the plain conv2 pool with inputs in [-16, 16] instead
    of [-2, 2] has values past 2^24 grains and no longer passes."""
    with pytest.raises(AssertionError):
        _check_model(X.pool32x(2, 0, 'plain', kmax=16))


@pytest.mark.parametrize('var', ['subw', 'sublo'])
@pytest.mark.parametrize('layer', [2, 3, 4])
def test_flushed_subnormal_halves_would_change_the_expectation(layer, var):
    """The subnormal pools decide what they are for: the model with every
    fp16-subnormal half flushed to zero (what an MFMA that dropped them would
    compute) moves most outputs by at least a grain of their 2^-15 grid."""
    pool = X.pool32x(layer, 0, var)
    st = X.GEOM[layer][4]
    flush = (lambda t: torch.where(t.abs() < FP16_MIN_NORMAL, torch.zeros_like(t), t))
    nchw = (lambda q: flush(q).permute(0, 3, 1, 2))
    acc0, acc1, _, _ = X.model3(nchw(pool['xh']), nchw(pool['xl']), flush(pool['th']),
                                flush(pool['tl']), st)
    moved = ((acc0 + acc1 / X.LO - pool['comb']) *
             2.0 ** pool['e'].double()[:, None, None, None]).abs()
    rows = [co for co in range(32) if co not in X.ZERO_CO]
    assert (moved[:, rows] >= 2.0 ** -15).double().mean().item() >= 0.5
