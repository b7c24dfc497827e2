"""DDPG update (aido1_amd/trainer.py) against the reference's own
DDPGTrainer.update: tests/golden/ddpg_update{,_f64}.json hold three updates of
the config.json actor/critic in train mode on a formula batch (dropout p=0 so
the run is deterministic), in float32 and in float64.

Why two precisions: after the first Adam step this update is chaotic in
float32.  The conv biases feed LeakyReLU -> train-mode BatchNorm, so their
gradients sit near zero, and Adam turns any gradient into a ~lr step whose
sign follows rounding noise; one-ulp differences (e.g. torch's capturable vs
plain Adam, tools/graph_probe.py) grow to percent-level loss differences by
the third update.  So: float64 pins all three updates tightly; float32 pins
the first update tightly and bounds the rest.  CPU here;
tests/test_gpu_trainer.py repeats the float32 check on the GPU.  Gradient
magnitudes, which Adam's sign-like first step hides, are pinned by
tests/test_update_ref.py (CPU) and tests/test_gpu_update_grads.py (GPU)."""
import copy
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
from formulas import formula_batch, formula_state_dict, param_summary  # noqa: E402


def no_dropout(net_config):
    net_config = copy.deepcopy(net_config)
    for part in net_config:
        for branch in part.get('modules', []):
            for m in branch:
                if m['name'] == 'dropout':
                    m['args']['p'] = 0.0
    return net_config


def make_trainer(device, double=False, **kw):
    from aido1_amd.actor import ConfigActor, ConfigCritic
    from aido1_amd.trainer import DDPGTrainer
    cfg = golden('reference_config.json')
    actor = ConfigActor(no_dropout(cfg['model']['actor']))
    critic = ConfigCritic(no_dropout(cfg['model']['critic']))
    actor.load_state_dict(formula_state_dict(actor.state_dict()))
    critic.load_state_dict(formula_state_dict(critic.state_dict()))
    if double:
        actor.double()
        critic.double()
    return DDPGTrainer(cfg, actor, critic, device=device, **kw)


def check_against_reference(tr, batch, rtol, atol, fixture='ddpg_update.json', later_rtol=0.1):
    """Update 1 to rtol/atol; updates 2-3 to later_rtol (the float32 drift
    described above; pass later_rtol=rtol for float64)."""
    ref = golden(fixture)
    for k in range(3):
        metrics, info = tr.update(batch)
        r = rtol if k == 0 else later_rtol
        a = atol if k == 0 else later_rtol
        np.testing.assert_allclose(metrics['critic_loss'].item(), ref['critic_loss'][k], rtol=r)
        np.testing.assert_allclose(metrics['actor_loss'].item(), ref['actor_loss'][k], rtol=r)
        np.testing.assert_allclose(info['td_error'].cpu().numpy().reshape(-1), ref['td_error'][k],
                                   rtol=r, atol=a)
    if later_rtol == rtol:          # float64: every parameter element tight,
        for name in ('actor', 'critic', 'target_actor', 'target_critic'):
            got = param_summary(getattr(tr, name))
            assert list(got) == list(ref[name]), name
            for key, vals in ref[name].items():
                # except the conv biases (near-zero gradients: even float64
                # runs differ at ~1e-7 with the CPU's thread-order reductions)
                # and the BatchNorm running means that carry them
                a_ = 1e-5 if key.endswith(('kernel.bias', 'running_mean')) else atol
                np.testing.assert_allclose(got[key], vals, rtol=rtol, atol=a_,
                                           err_msg=name + key)
        return
    # Parameters are [sum, abs-sum, 32 elements] per tensor.  Adam's first
    # steps move each weight by about +-lr whatever the gradient's size, and
    # the conv biases feeding a train-mode BatchNorm get gradients close to
    # zero, so a different summation order can flip their step: any element
    # may differ by up to 2 * lr per update (3 updates, lr <= 0.004), and
    # >= 90% of them must agree to the tight tolerance.
    bound = 2 * 3 * 0.004 + atol
    close, total = 0, 0
    for name in ('actor', 'critic', 'target_actor', 'target_critic'):
        got = param_summary(getattr(tr, name))
        assert list(got) == list(ref[name]), name           # reference state_dict keys
        for key, vals in ref[name].items():
            # (entry 0, the plain sum, accumulates those flips over up to 1M
            # weights and is not compared in float32; for the conv biases,
            # whose gradients are all near zero, neither is entry 1, the
            # abs-sum: 32 elements may each flip -- nor for the BatchNorm
            # running means, which carry those biases, as the float64 branch
            # above treats them)
            skip = 2 if key.endswith(('kernel.bias', 'running_mean')) else 1
            g, r = np.asarray(got[key])[skip:], np.asarray(vals)[skip:]
            d = np.abs(g - r)
            assert d.max() <= bound + rtol * np.abs(r).max(), (name + key, d.max())
            close += int(np.sum(d <= atol + rtol * np.abs(r)))
            total += d.size
    assert close >= 0.9 * total, (close, total)


def test_update_matches_reference_cpu():
    tr = make_trainer('cpu')
    check_against_reference(tr, formula_batch(16), rtol=1e-4, atol=1e-4)
    assert tr.global_update_step == 3


def test_update_matches_reference_f64_cpu():
    tr = make_trainer('cpu', double=True)
    check_against_reference(tr, formula_batch(16), rtol=1e-8, atol=1e-9,
                            fixture='ddpg_update_f64.json', later_rtol=1e-8)


def test_critic_forward_and_keys():
    from aido1_amd.actor import ConfigCritic
    from formulas import formula_input, hash_u
    g = golden('actor.npz')
    cr = ConfigCritic(golden('reference_config.json')['model']['critic'])
    assert list(cr.state_dict().keys()) == list(g['config_critic_keys'])
    assert sum(p.numel() for p in cr.parameters()) == 1121409
    cr.load_state_dict(formula_state_dict(cr.state_dict()))
    cr.eval()
    with torch.no_grad():
        y = cr(formula_input(4), hash_u(8, 77).reshape(4, 2).float())
    np.testing.assert_allclose(y.numpy(), g['config_critic'], rtol=1e-5, atol=1e-6)


def test_soft_update_expression():
    from aido1_amd.trainer import soft_update
    a, b = torch.nn.Linear(64, 64), torch.nn.Linear(64, 64)
    ta = copy.deepcopy(a)
    tau = 1e-4
    expect = [t.data * (1.0 - tau) + p.data * tau for t, p in zip(ta.parameters(), b.parameters())]
    soft_update(ta, b, tau)
    for t, e in zip(ta.parameters(), expect):
        assert torch.equal(t.data, e)


@pytest.mark.parametrize('kind', ['adamw', 'sgd'])
def test_other_optimizers_step(kind):
    from aido1_amd.optim import make_optimizer
    lin = torch.nn.Linear(4, 2)
    opt = make_optimizer(kind, lin.parameters())
    opt.param_groups[0]['lr'] = 0.1
    lin(torch.ones(3, 4)).sum().backward()
    w0 = lin.weight.detach().clone()
    opt.step()
    assert not torch.equal(lin.weight, w0)
