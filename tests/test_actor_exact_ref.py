"""The conditions under which tests/test_gpu_actor_exact.py may demand bit
equality of the fp16 actor convolutions, asserted on every pool it uses
(tests/actor_exact_ref.py), the degenerate channels the pools must hold, and
the constants of the tolerances that remain.  These are caps, not measurements:
a pool that breaks one of them makes the GPU equality meaningless."""
import numpy as np
import pytest
import torch

import actor_exact_ref as R

POOLS32 = [(layer, seed, eps) for layer in (2, 3, 4) for seed, eps in R.VARIANTS]
IDS32 = ['conv%d-set%d-eps%g' % p for p in POOLS32]
LIMIT = 2.0 ** 24


def _is_grid(t, grain):
    return bool((t / grain == torch.round(t / grain)).all())


def _f32_exact(t):
    return bool((t.float().double() == t).all())


def _cases(pool):
    """(name, accumulators, sum of |terms|, grain of the terms, stored values)."""
    if pool['layer'] == 1:
        return [('ref', pool['acc'], pool['terms'], 1 / 32, pool['d']),
                ('eval', pool['acc'], pool['terms'], 1 / 32, pool['v'])]
    out = [('ref', pool['acc'], pool['terms'], 1 / 16, pool['d'])]
    if 'ye' in pool:      # eval mode stages the same values without a norm
        out.append(('eval', pool['acce'], pool['terms'] + 3 / 32, 1 / 32, pool['ve']))
    return out


def _check_exactness(pool):
    for name, acc, terms, grain, stored in _cases(pool):
        # every term on the grain, the sum of their magnitudes below 2^24 grains:
        # each partial sum is an integer of grains below 2^24, exact in float32
        assert _is_grid(acc, grain), name
        assert (terms / grain).max().item() < LIMIT, name
        # LeakyReLU's product, the centre and the centred value are float32 numbers
        assert _f32_exact(R.lrelu(acc)) and _f32_exact(stored), name
        assert torch.isfinite(stored.float().half()).all(), name
        neg, pos = (acc < 0).double().mean().item(), (acc > 0).double().mean().item()
        assert neg >= 0.25 and pos >= 0.25, (name, neg, pos)
    assert _f32_exact(pool['v']) and _f32_exact(pool['c']) and _f32_exact(pool['d'])


@pytest.mark.parametrize('layer,seed,eps', POOLS32, ids=IDS32)
def test_conv32_pools_keep_float32_arithmetic_exact(layer, seed, eps):
    pool = R.pool32(layer, seed, eps)
    st = pool['staged']
    assert torch.equal(st.half().double(), st)          # staged inputs are fp16 numbers
    assert _is_grid(st, 1 / 16) and st.abs().max().item() <= 17
    x = pool['x16'].double()
    assert _is_grid(x, 1.0) and x.abs().max().item() <= 3
    assert _is_grid(pool['w'].double(), 1.0) and pool['w'].abs().max().item() == 1
    assert (pool['w'] == 0).double().mean().item() >= 0.5
    assert _is_grid(pool['b'].double(), 0.25)
    _check_exactness(pool)
    # the store's rounding is exercised: some, not most, values are not fp16 numbers
    for name, _, _, _, stored in _cases(pool):
        inexact = (stored.float().half().double() != stored).double().mean().item()
        assert 0.05 <= inexact <= 0.50, (name, inexact)
    # distinct samples: a gather by the wrong index cannot pass
    y = pool['y'].view(torch.int16)
    for i in range(R.P):
        for j in range(i):
            assert not torch.equal(y[i], y[j])
            assert not torch.equal(pool['prev'][i], pool['prev'][j])


@pytest.mark.parametrize('seed', [0, 1])
def test_conv1_pools_keep_float32_arithmetic_exact(seed):
    pool = R.pool1(seed)
    fr = pool['frames'].double()
    assert torch.equal(fr.half().double(), fr)
    assert _is_grid(fr, 1 / 8) and fr.min().item() >= 0 and fr.max().item() <= 1
    assert _is_grid(pool['w'].double(), 0.25) and pool['w'].abs().max().item() <= 0.5
    assert _is_grid(pool['b'].double(), 0.25)
    _check_exactness(pool)
    # every stored value is an fp16 number (the issue's measurement, as a cap)
    assert torch.equal(pool['y'].double(), pool['d'].permute(0, 2, 3, 1))
    assert torch.equal(pool['ye'].double(), pool['v'].permute(0, 2, 3, 1))


@pytest.mark.parametrize('layer,seed,eps', POOLS32, ids=IDS32)
def test_norm_of_the_pools_is_dyadic_in_the_kernels_float32(layer, seed, eps):
    """stats_merge restated in float32 (norm32): sc and sh are exact powers of
    two times small integers, except the eps variant's flat channel."""
    pool = R.pool32(layer, seed, eps)
    ih, iw = R.GEOM[layer][:2]
    prev = pool['prev'].numpy()
    sc, sh = R.norm32(prev, pool['gamma'].numpy(), pool['beta'].numpy(), eps, ih * iw)
    dyadic = np.frexp(sc)[0] == 0.5
    assert sc.min() >= 0.25 or eps
    if eps:
        assert not dyadic[:, R.FLAT_CI].any()                 # gamma / sqrt(eps)
        assert (prev[:, R.FLAT_CI, :2] == 0).all()
        assert (pool['x16'][..., R.FLAT_CI] == 0).all()
        beta = pool['beta'][R.FLAT_CI].double()
        assert beta != 0
        assert (pool['staged'][..., R.FLAT_CI] == beta).all()   # exactly beta all the same
        dyadic = np.delete(dyadic, R.FLAT_CI, 1)
        sc = np.delete(sc, R.FLAT_CI, 1)
    assert dyadic.all() and sc.min() >= 0.25 and sc.max() <= 4
    assert _is_grid(torch.from_numpy(sh.astype(np.float64)), 1 / 16)


@pytest.mark.parametrize('layer', [1, 2, 3, 4])
def test_degenerate_output_channels_are_in_the_pools(layer):
    pools = [R.pool1(0), R.pool1(1)] if layer == 1 else [R.pool32(layer, s, e)
                                                         for s, e in R.VARIANTS]
    for pool in pools:
        for co, sign in zip(R.ZERO_CO, (1, -1)):
            assert (pool['w'][co] == 0).all() and pool['b'][co].item() * sign > 0
            want_c = R.lrelu(pool['b'][co].double())
            assert (pool['c'][:, co] == want_c).all()
            assert (pool['y'][..., co] == 0).all()
            if layer != 4:
                part = pool['part'][:, co]
                assert (part[:, :2] == 0).all() and (part[:, 2] == want_c).all()
                assert (pool['mean32'][:, co] == 0).all() and (pool['m2_32'][:, co] == 0).all()
            else:   # conv4's own BatchNorm of a flat channel: exactly out_beta
                ob = pool['ob'][co]
                assert ob.item() * sign > 0
                assert (pool['want'].view(R.P, 32, -1)[:, co] == ob.double()).all()
                out32 = pool['out32'].view(R.P, 32, -1)[:, co]
                assert (out32.float().half() == ob.half()).all()


def test_bound_constants_are_four_times_cpu_float32():
    """K_STAT and K_OUT4 are four times the float32 restatements' worst error
    against float64 on the pools the GPU tests use (the helper's docstring has
    the figures), rounded up by less than a tenth."""
    worst = {1: [0.0, 0.0], 2: [0.0, 0.0], 3: [0.0, 0.0]}
    pools = [R.pool1(0), R.pool1(1)] + [R.pool32(layer, s, e) for layer in (2, 3)
                                        for s, e in R.VARIANTS]
    for pool in pools:
        e = R.stat_units(pool)
        print(pool['layer'], e)
        worst[pool['layer']] = [max(a, b) for a, b in zip(worst[pool['layer']], e)]
    for layer, w in worst.items():
        for k, e in zip(R.K_STAT[layer], w):
            assert 4 * e <= k <= 4.1 * e + 0.05, (layer, k, e)
    e4 = max(R.out4_units(R.pool32(4, s, e)) for s, e in R.VARIANTS)
    print(4, e4)
    assert 4 * e4 <= R.K_OUT4 <= 4.1 * e4 + 0.05, e4


def test_welford32_follows_float64_on_random_values():
    """The restatement is a statistics routine in its own right: on values with
    a large offset it stays within a few u of the float64 mean and M2 (in the
    offset's units), for every layer's pixel count and wave count."""
    rng = np.random.default_rng(3)
    for layer in (1, 2, 3):
        oh, ow, waves = R.GEOM[layer][2], R.GEOM[layer][3], R.GEOM[layer][5]
        d = (rng.standard_normal((2, 4, oh * ow)) + 10.0).astype(np.float32)
        mean, m2 = R.welford32(d, waves)
        d64 = d.astype(np.float64)
        m64 = d64.mean(-1)
        q64 = ((d64 - m64[..., None]) ** 2).sum(-1)
        assert np.abs(mean - m64).max() <= 8 * R.U * 14
        assert np.abs(m2 - q64).max() <= 8 * R.U * (oh * ow) * 14 + 64 * R.U * q64.max()


@pytest.mark.parametrize('layer', [2, 3, 4])
def test_one_tap_error_hides_under_the_max_abs_tolerance(layer):
    """The sensitivity test's perturbation (one tap of one (co, ci) pair moved
    by TAP_GRAIN) changes the outputs by less than the 3e-3 max(1, max |ref|)
    of test_conv32_layers_match_conv2d, and still changes stored fp16 bits, in
    channel co alone: the equality sees what that tolerance cannot."""
    pool = R.pool32(layer, 0, 0.0)
    co = 9
    _, v = R.perturbed_tap(pool, co=co)
    ref = pool['v']
    err = (v - ref).abs()
    assert 0 < err.max().item() < 3e-3 * max(1.0, ref.abs().max().item())
    d = v - v[:, :, :1, :1]
    bits = d.float().half().view(torch.int16) != pool['d'].float().half().view(torch.int16)
    assert bits[:, co].any()
    bits[:, co] = False
    assert not bits.any()
    # the perturbed problem is still exact: TAP_GRAIN x the 1/16 grid, far below 2^24
    assert (pool['terms'] * 16 / R.TAP_GRAIN).max().item() < LIMIT
