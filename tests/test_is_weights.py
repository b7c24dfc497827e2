"""Importance weights of the prioritized replay in the critic loss, without a
GPU: DDPGTrainer(importance_weights=True) against the update written out in
plain autograd (float64), ones against no weights, the switches' errors,
train_loop.beta_schedule, and the new entry points' host argument checks.
The kernels and the GPU paths are tests/test_gpu_is_weights.py."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_trainer import formula_batch, make_trainer

KINDS = ['mse_loss', 'smooth_l1_loss']


def fixed_weights(n=16):
    """w_i = ((7 i mod n) + 1) / n: every value of 1/n .. 1 once, not sorted."""
    return ((7 * np.arange(n)) % n + 1) / float(n)


def kind_trainer(device, kind, **kw):
    tr = make_trainer(device, **kw)
    tr.critic_loss_kind = kind
    return tr


@pytest.mark.parametrize('kind', KINDS)
def test_weighted_update_equals_plain_autograd_f64(kind):
    """One float64 update with the fixed weights against the same update
    written out on copies of the networks: target actor -> target critic -> y,
    the critic's forward, (w * loss_i).mean(), torch.autograd.grad.  Both sides
    run the same float64 torch ops; the tolerance covers thread-order
    reductions only."""
    tr = kind_trainer('cpu', kind, double=True, importance_weights=True)
    nets = {n: copy.deepcopy(getattr(tr, n)) for n in ('critic', 'target_actor', 'target_critic')}
    obs, act, rew, nxt, done = formula_batch(16)
    w = fixed_weights()
    metrics, info = tr.update((obs, act, rew, nxt, done), weights=w)

    cl = torch.channels_last
    t = lambda x: torch.as_tensor(x).double()
    obs_t, nxt_t = t(obs).contiguous(memory_format=cl), t(nxt).contiguous(memory_format=cl)
    rew_t, w_t = t(rew).reshape(-1, 1), t(w).reshape(-1, 1)
    notdone = (~torch.as_tensor(done).reshape(-1, 1)).double()
    with torch.no_grad():
        next_v = nets['target_critic'](nxt_t, nets['target_actor'](nxt_t))
        y = rew_t + notdone * tr.gamma * next_v
    q = nets['critic'](obs_t, t(act))
    if kind == 'mse_loss':
        terms = (q - y) ** 2
    else:
        terms = F.smooth_l1_loss(q, y, reduction='none')
    loss = (w_t * terms).mean()
    params = list(nets['critic'].parameters())
    grads = torch.autograd.grad(loss, params)

    tol = dict(rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(metrics['critic_loss'].item(), torch.sqrt(loss).item(), **tol)
    names = [n for n, _ in nets['critic'].named_parameters()]
    got = dict(tr.critic.named_parameters())
    assert tr._in['w'].dtype == torch.float64 and tuple(tr._in['w'].shape) == (16, 1)
    for n, g in zip(names, grads):
        np.testing.assert_allclose(got[n].grad.numpy(), g.numpy(), err_msg=n, **tol)
    # td_error stays the raw y - Q(s, a) of the stepped critic (train-mode
    # BatchNorm: its output does not depend on the running statistics the
    # update's own forwards moved)
    with torch.no_grad():
        td = y - copy.deepcopy(tr.critic)(obs_t, t(act))
    np.testing.assert_allclose(info['td_error'].numpy(), td.numpy(), **tol)


@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('kind', KINDS)
def test_ones_equal_no_weights(kind, double):
    """weights=None, weights of ones, and a trainer without the switch: the
    same losses and TD errors over 3 updates."""
    trs = [kind_trainer('cpu', kind, double=double, importance_weights=True),
           kind_trainer('cpu', kind, double=double, importance_weights=True),
           kind_trainer('cpu', kind, double=double)]
    batch = formula_batch(16)
    ws = [{}, {'weights': np.ones(16, np.float32)}, {}]
    for _ in range(3):
        out = [tr.update(batch, **kw) for tr, kw in zip(trs, ws)]
        for m, info in out[1:]:
            for key in ('critic_loss', 'actor_loss'):
                np.testing.assert_allclose(m[key].item(), out[0][0][key].item(), rtol=1e-12,
                                           err_msg=key)
            np.testing.assert_allclose(info['td_error'].numpy(), out[0][1]['td_error'].numpy(),
                                       rtol=1e-12)
    assert 'w' in trs[0]._in and 'w' not in trs[2]._in


def test_weights_matter_and_switches_are_enforced():
    batch = formula_batch(16)
    w = fixed_weights()
    plain = make_trainer('cpu')
    weighted = make_trainer('cpu', importance_weights=True)
    a = plain.update(batch)[0]['critic_loss'].item()
    for shape in ((16,), (16, 1)):          # [b] and [b, 1], numpy and tensor, any float dtype
        for conv in (np.asarray, lambda v: torch.as_tensor(v, dtype=torch.float16)):
            tr = make_trainer('cpu', importance_weights=True)
            b = tr.update(batch, weights=conv(w.reshape(shape)))[0]['critic_loss'].item()
            assert abs(b - a) > 1e-3 * abs(a), (a, b)
    with pytest.raises(ValueError):
        plain.update(batch, weights=w)
    with pytest.raises(ValueError):
        weighted.update(batch, weights=w[:8])
    from aido1_amd import train_ops
    x = torch.zeros(4, 1)
    with pytest.raises(ValueError):
        train_ops.weighted_loss(x, x, x, 'neg_mean')


def test_beta_schedule():
    from aido1_amd.train_loop import beta_schedule
    t = {'beta': 0.5}
    lin = beta_schedule(t, {'type': 'linear', 'args': {'initial_value': 0.4, 'final_value': 1.0,
                                                       'max_step': 100}})
    for step, want in ((0, 0.4), (50, 0.7), (100, 1.0)):
        assert lin(step) == pytest.approx(want, rel=1e-12)
    assert lin(150) == 1.0                                   # capped, not 1.3
    const = beta_schedule(t, None)
    assert [const(s) for s in (0, 7, 10 ** 6)] == [0.5] * 3


def test_entry_points_check_arguments():
    """dt_loss_w / dt_loss_w_bwd / dt_frame_gather_w are exported, bound at ABI
    14, and refuse bad host arguments before any GPU work (DT_E_ARG, -1)."""
    from aido1_amd import _lib
    L = _lib.lib()
    assert L.dt_abi_version() == _lib.ABI_VERSION == 14
    assert {'dt_loss_w', 'dt_loss_w_bwd', 'dt_frame_gather_w'} <= set(_lib.exported_symbols())
    one = (ctypes.c_double * 1)(0.0)
    p = ctypes.addressof(one)           # any non-null address: never dereferenced here
    for kind in (1, 3, -1):
        assert L.dt_loss_w(kind, 4, p, p, p, p, None) == -1
        assert L.dt_loss_w_bwd(kind, 4, p, p, p, p, p, None) == -1
    for kind in (0, 2):
        assert L.dt_loss_w(kind, 0, p, p, p, p, None) == -1
        assert L.dt_loss_w_bwd(kind, 0, p, p, p, p, p, None) == -1
        for k in (0, 1, 3):             # a, b, loss (w, at 2, may be NULL)
            args = [p] * 4
            args[k] = None
            assert L.dt_loss_w(kind, 4, *args, None) == -1
        for k in (0, 1, 3, 4):          # a, b, g, da
            args = [p] * 5
            args[k] = None
            assert L.dt_loss_w_bwd(kind, 4, *args, None) == -1
    gather = lambda weights, w: L.dt_frame_gather_w(1, p, p, 0, 16, 3, p, p, p, p, p, p, p, p, p,
                                                    p, weights, w, None)
    assert gather(p, None) == -1
    assert gather(None, p) == -1
