"""The device optimisers' host side (aido1_amd/optim.py DeviceAdamW / DeviceSGD,
include/dttrain.h dt_adamw / dt_sgd), without a GPU: what make_optimizer
returns off the GPU, the entry points' argument checks, and the trainer on the
CPU.  The kernels themselves are tests/test_gpu_optim_device.py."""
import ctypes

import numpy as np
import pytest
import torch

from test_trainer import formula_batch, make_trainer, param_summary

KINDS = ['adamw', 'sgd']


def _host_class(kind):
    from aido1_amd.optim import AdamW
    return AdamW if kind == 'adamw' else torch.optim.SGD


@pytest.mark.parametrize('kind', KINDS)
def test_make_optimizer_off_the_gpu_is_the_host_class(kind):
    """Without capturable, and with capturable on the CPU, "adamw" and "sgd"
    are the host classes with the reference's hyper-parameters, lr a float 0."""
    from aido1_amd.optim import DeviceStep, make_optimizer
    for kw in ({}, dict(capturable=True, device='cpu'), dict(capturable=False, device='cpu')):
        opt = make_optimizer(kind, torch.nn.Linear(4, 2).parameters(), **kw)
        assert type(opt) is _host_class(kind) and not isinstance(opt, DeviceStep)
        g = opt.param_groups[0]
        assert g['lr'] == 0.0 and not torch.is_tensor(g['lr']) and g['weight_decay'] == 1e-4
        if kind == 'sgd':
            assert g['momentum'] == 0.9


def test_unknown_kind_is_refused():
    from aido1_amd.optim import make_optimizer
    with pytest.raises(NotImplementedError):
        make_optimizer('rmsprop', torch.nn.Linear(4, 2).parameters(), capturable=True,
                       device='cpu')


def test_entry_points_check_arguments():
    """dt_adamw / dt_sgd are exported, bound at ABI 14, and check their host
    arguments before any GPU work: a negative chunk count or null tables are
    DT_E_ARG (-1), no chunks is DT_OK (0) with nothing launched."""
    from aido1_amd import _lib
    L = _lib.lib()
    assert L.dt_abi_version() == _lib.ABI_VERSION == 14
    assert {'dt_adamw', 'dt_sgd'} <= set(_lib.exported_symbols())
    one = (ctypes.c_double * 1)(0.0)
    tab = ctypes.addressof(one)         # any non-null address: never dereferenced here
    adamw = lambda n, t, c, s, lr, k: L.dt_adamw(n, t, c, s, lr, 0.9, 0.999, 1e-8, 1e-4, k,
                                                 None, -1, -1, None)
    sgd = lambda n, t, c, lr: L.dt_sgd(n, t, c, lr, 0.9, 1e-4, None, -1, -1, None)
    assert adamw(-1, tab, tab, tab, tab, tab) == -1
    assert adamw(0, None, None, None, None, None) == 0
    assert sgd(-1, tab, tab, tab) == -1
    assert sgd(0, None, None, None) == 0
    for k in range(5):                  # one null among (tensors, chunks, step, lr, counter)
        args = [tab] * 5
        args[k] = None
        assert adamw(1, *args) == -1
    for k in range(3):                  # (tensors, chunks, lr)
        args = [tab] * 3
        args[k] = None
        assert sgd(1, *args) == -1


def _cfg_trainer(kind, **kw):
    """test_trainer.make_trainer with training.optimizer = kind (make_trainer
    reads the golden config itself, so the same construction here)."""
    from conftest import golden
    from aido1_amd.actor import ConfigActor, ConfigCritic
    from aido1_amd.trainer import DDPGTrainer
    from test_trainer import formula_state_dict, no_dropout
    cfg = golden('reference_config.json')
    cfg['training']['optimizer'] = kind
    actor = ConfigActor(no_dropout(cfg['model']['actor']))
    critic = ConfigCritic(no_dropout(cfg['model']['critic']))
    actor.load_state_dict(formula_state_dict(actor.state_dict()))
    critic.load_state_dict(formula_state_dict(critic.state_dict()))
    return DDPGTrainer(cfg, actor, critic, **kw)


@pytest.mark.parametrize('kind', KINDS)
def test_cpu_trainer_with_graph_requested(kind):
    """graph=True on the CPU is forced off and the host optimiser steps; two
    such trainers agree exactly after an update (the floor under the GPU
    suite's comparison with this trainer)."""
    trs = [_cfg_trainer(kind, device='cpu', graph=True) for _ in range(2)]
    for tr in trs:
        assert tr.graph is False and type(tr.actor_optim) is _host_class(kind)
        tr.update(formula_batch(16))
    for name in ('actor', 'critic', 'target_actor', 'target_critic'):
        a, b = (param_summary(getattr(tr, name)) for tr in trs)
        assert list(a) == list(b)
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), name + key
    w = trs[0].actor.net.input_nets[0].internal_modules[0].kernel.weight
    assert not torch.equal(w, make_trainer('cpu').actor.net.input_nets[0].internal_modules[0]
                           .kernel.weight)


def test_cpu_trainer_refuses_unknown_kind():
    with pytest.raises(NotImplementedError):
        _cfg_trainer('rmsprop', device='cpu', graph=True)
