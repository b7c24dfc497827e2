"""One DDPG update (training/trainers.py:156-229) written out in plain float64
torch on the CPU, in the reference's order and with full forwards: no shared
trunk, three critic forwards an update, no fused kernel.  It imports nothing of
aido1_amd.trainer, so the trainer's stages (and the kernels under them) can be
held to it: tests/test_update_ref.py (the restatement itself and the CPU
float32 yardstick), tests/test_gpu_update_grads.py (the eager GPU stages).

Also here, shared by those two files: the cases (batch, loss, weights,
learning rates), the reference run of a case (computed once and left
unchanged), and the error units."""
import copy
import functools
import sys

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
from formulas import formula_batch, formula_state_dict  # noqa: E402

NETS = ('actor', 'critic', 'target_actor', 'target_critic')
U = 2.0 ** -24


def ddpg_update_ref(nets, batch, opts, lrs, gamma, tau, kind='mse_loss', weights=None):
    """nets: dict of the four float64 train-mode networks; batch: (obs,
    actions, rewards, next_obs, dones); opts: {'critic', 'actor'} host
    optimisers over nets['critic'] / nets['actor']; lrs: their learning rates
    at this update.  -> y, critic_loss, actor_loss, td, the gradients by
    parameter name ('critic_grads', 'actor_grads') and the four state_dicts
    after the update, all detached float64 copies."""
    actor, critic = nets['actor'], nets['critic']
    t = lambda v: torch.as_tensor(v).double()
    obs, act, rew, nxt = t(batch[0]), t(batch[1]), t(batch[2]).reshape(-1, 1), t(batch[3])
    notdone = (~torch.as_tensor(batch[4], dtype=torch.bool).reshape(-1, 1)).double()
    w = torch.ones_like(rew) if weights is None else t(weights).reshape(-1, 1)

    def grads_of(name, loss):
        params = dict(nets[name].named_parameters())
        return dict(zip(params, torch.autograd.grad(loss, list(params.values()))))

    def step(name, grads):
        for n, p in nets[name].named_parameters():
            p.grad = grads[n].clone()
        opts[name].param_groups[0]['lr'] = lrs[name]
        opts[name].step()

    with torch.no_grad():
        y = rew + notdone * gamma * nets['target_critic'](nxt, nets['target_actor'](nxt))
    q = critic(obs, act)
    if kind == 'mse_loss':
        terms = (q - y) ** 2
    elif kind == 'smooth_l1_loss':
        terms = F.smooth_l1_loss(q, y, reduction='none')
    else:
        raise NotImplementedError(kind)
    critic_loss = (w * terms).mean()
    d0 = (y - q).detach()                       # before the step: the loss's arguments
    critic_grads = grads_of('critic', critic_loss)
    step('critic', critic_grads)
    actor_loss = -critic(obs, actor(obs)).mean()
    actor_grads = grads_of('actor', actor_loss)
    with torch.no_grad():
        td = y - critic(obs, act)
    step('actor', actor_grads)
    with torch.no_grad():
        for tn, sn in (('target_actor', 'actor'), ('target_critic', 'critic')):
            for tp, sp in zip(nets[tn].parameters(), nets[sn].parameters()):
                tp.copy_(tp * (1.0 - tau) + sp * tau)
    return {'y': y.clone(), 'd0': d0, 'critic_loss': critic_loss.detach().clone(),
            'actor_loss': actor_loss.detach().clone(), 'td': td.clone(),
            'critic_grads': critic_grads, 'actor_grads': actor_grads,
            'state': {n: {k: v.detach().clone() for k, v in nets[n].state_dict().items()}
                      for n in NETS}}


# ---- the networks, the config and the cases -----------------------------------------------
def no_dropout(net_config):
    net_config = copy.deepcopy(net_config)
    for part in net_config:
        for branch in part.get('modules', []):
            for m in branch:
                if m['name'] == 'dropout':
                    m['args']['p'] = 0.0
    return net_config


def float64_nets(cfg):
    """The four networks as test_trainer.make_trainer builds them, in float64
    and train mode."""
    from aido1_amd.actor import ConfigActor, ConfigCritic
    actor = ConfigActor(no_dropout(cfg['model']['actor']))
    critic = ConfigCritic(no_dropout(cfg['model']['critic']))
    actor.load_state_dict(formula_state_dict(actor.state_dict()))
    critic.load_state_dict(formula_state_dict(critic.state_dict()))
    nets = {'actor': actor.double(), 'critic': critic.double()}
    nets['target_actor'] = copy.deepcopy(nets['actor'])
    nets['target_critic'] = copy.deepcopy(nets['critic'])
    for m in nets.values():
        m.train()
    return nets


LR_SCALE = 2.0 ** -10


def case_config(optimizer, scaled):
    """The golden config with training.optimizer = `optimizer`; scaled: both
    learning-rate decays times 2^-10 (the formula weights give critic
    gradients of order 1e2, for which the config's step is so large that a
    second float32 update is no longer comparable with a float64 one)."""
    cfg = golden('reference_config.json')
    cfg['training']['optimizer'] = optimizer
    if scaled:
        for key in ('actor_train_decay', 'critic_train_decay'):
            args = cfg['training'][key]['lr']['args']
            args['initial_value'] *= LR_SCALE
            args['final_value'] *= LR_SCALE
    return cfg


def lrs_at(cfg, step):
    """utils/util.py:77-90 with config.json's linear decay."""
    out = {}
    for name in ('actor', 'critic'):
        c = cfg['training'][name + '_train_decay']['lr']
        assert c['type'] == 'linear'
        i, f, m = c['args']['initial_value'], c['args']['final_value'], c['args']['max_step']
        rel = 1.0 - step / m
        out[name] = i * rel + f * (1.0 - rel)
    return out


# (batch, loss kind, importance weights, scaled learning rates, updates).
# Batches: 5 is no multiple of any tile, 16 the goldens'; 62 and 65 are on
# either side of the fused MLP tail's limit for the critic's head
# (train_ops.mlp_plan: m * n1 = m * 128 <= 8192, i.e. m <= 64).  Why these two
# and why one update each: tests/test_update_ref.py, "LeakyReLU's kink".  The
# config's learning rates run one update, the scaled ones two where that test
# allows a second.
LOSS_CASES = [(5, 'mse_loss', False, True, 2), (16, 'mse_loss', False, True, 2),
              (62, 'mse_loss', False, True, 1), (65, 'mse_loss', False, True, 1),
              (16, 'mse_loss', False, False, 1),
              (16, 'mse_loss', True, True, 2), (16, 'smooth_l1_loss', True, True, 1)]
GRAD_FIGURES = ('critic_grad', 'critic_grad_l2', 'actor_grad', 'actor_grad_l2')


def case_id(case):
    b, kind, weighted, scaled, updates = case
    return 'b%d-%s%s-%s-%dupd' % (b, kind.replace('_loss', ''), '-w' if weighted else '',
                                  'lr_scaled' if scaled else 'lr_config', updates)


def case_updates(case):
    return case[4]


def case_weights(case):
    """test_is_weights.fixed_weights: every value of 1/n .. 1 once, not sorted."""
    from test_is_weights import fixed_weights
    return fixed_weights(case[0]) if case[2] else None


def host_optimizer(kind, params):
    """optim.make_optimizer's host classes (training/trainers.py:258-268)."""
    from aido1_amd.optim import make_optimizer
    return make_optimizer(kind, params)


def run_reference(cfg, batch, updates, kind='mse_loss', weights=None):
    """`updates` updates of ddpg_update_ref from the formula weights with
    cfg's optimiser, gamma, tau and learning rates -> (the list of its
    outputs, the networks afterwards)."""
    nets = float64_nets(cfg)
    t = cfg['training']
    opts = {n: host_optimizer(t['optimizer'], nets[n].parameters()) for n in ('critic', 'actor')}
    outs = [ddpg_update_ref(nets, batch, opts, lrs_at(cfg, k), float(t['gamma']),
                            float(t['tau']), kind, weights) for k in range(updates)]
    return outs, nets


@functools.lru_cache(maxsize=None)
def reference(case):
    """The float64 SGD reference of a case: computed once, read by every test."""
    b, kind, weighted, scaled, updates = case
    return run_reference(case_config('sgd', scaled), formula_batch(b), updates, kind,
                         case_weights(case))[0]


NUDGE = 1.0 + 8 * U


def nudged_reference(case):
    """reference(case) with both observation batches multiplied by 1 + 8 u: a
    perturbation of the size of float32 rounding.  Where its gradients differ
    from reference(case)'s by more than rounding, some pre-activation sits so
    close to LeakyReLU's kink that float32 arithmetic takes either branch, and
    no float32 update can be held to the float64 one on that input."""
    b, kind, weighted, scaled, updates = case
    obs, act, rew, nxt, done = formula_batch(b)
    batch = (obs.astype(np.float64) * NUDGE, act, rew, nxt.astype(np.float64) * NUDGE, done)
    return run_reference(case_config('sgd', scaled), batch, updates, kind, case_weights(case))[0]


# ---- error units --------------------------------------------------------------------------
def units(got, ref):
    """max |got - ref| in u * max |ref| (u = 2^-24).  No floor: an identically
    zero reference allows no error (inf otherwise)."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    if err == 0.0:
        return 0.0
    return err / (U * scale) if scale > 0.0 else float('inf')


def l2_units(got, ref):
    """||got - ref|| / ||ref|| in u."""
    got, ref = got.detach().double().cpu(), ref.double()
    err, scale = float((got - ref).norm()), float(ref.norm())
    if err == 0.0:
        return 0.0
    return err / (U * scale) if scale > 0.0 else float('inf')


KINDS_OF_FIGURE = ('y', 'critic_loss', 'actor_loss', 'td', 'critic_grad', 'critic_grad_l2',
                   'actor_grad', 'actor_grad_l2', 'state')


class Worst:
    """The worst figure of each kind, with the tensor it came from."""

    def __init__(self):
        self.fig = {k: (0.0, '') for k in KINDS_OF_FIGURE}

    def add(self, kind, value, where=''):
        if not value <= self.fig[kind][0]:          # a NaN counts as worst
            self.fig[kind] = (float(value), where)

    def merge(self, other):
        for k, (v, where) in other.fig.items():
            self.add(k, v, where)

    def __str__(self):
        return ', '.join('%s %.3g%s' % (k, v, ' (%s)' % w if w else '')
                         for k, (v, w) in self.fig.items())


def measure(worst, ref, y, critic_loss, actor_loss, td, critic_grads, actor_grads, states, tag=''):
    """One update's outputs against ddpg_update_ref's `ref`, into `worst`.
    critic_grads / actor_grads: dicts by parameter name; states: the four
    state_dicts by network name.  num_batches_tracked must be equal."""
    worst.add('y', units(y.reshape(-1, 1), ref['y']), tag)
    worst.add('td', units(td.reshape(-1, 1), ref['td']), tag)
    for k, v in (('critic_loss', critic_loss), ('actor_loss', actor_loss)):
        worst.add(k, units(torch.as_tensor(v).reshape(()), ref[k]), tag)
    for net, grads in (('critic', critic_grads), ('actor', actor_grads)):
        want = ref[net + '_grads']
        assert list(grads) == list(want), net
        for name, g in grads.items():
            worst.add(net + '_grad', units(g, want[name]), tag + name)
            worst.add(net + '_grad_l2', l2_units(g, want[name]), tag + name)
    for net in NETS:
        want = ref['state'][net]
        assert list(states[net]) == list(want), net
        for name, v in states[net].items():
            if name.endswith('num_batches_tracked'):
                assert int(v) == int(want[name]), (net, name, int(v), int(want[name]))
            else:
                worst.add('state', units(v, want[name]), tag + net + '.' + name)


# The bounds: 4 times the worst figure of the float32 CPU trainer over the
# cases at batches 5 and 16 (tests/test_update_ref.py has the figures and why
# the larger batches set no constant), in the units above.
K = {'y': 69.0, 'critic_loss': 107.0, 'actor_loss': 960.0, 'td': 188.0,
     'critic_grad': 1030.0, 'critic_grad_l2': 660.0, 'actor_grad': 1270.0,
     'actor_grad_l2': 1060.0, 'state': 904.0}
