"""The eager GPU stages of the DDPG update (DDPGTrainer._stage_critic /
_stage_actor / _stage_targets: the fused kernels stitched together, the shared
critic trunk under no_grad on a side stream, td_target, running_updates(critic,
2), _grads handing autograd outputs to the device optimiser) against the
float64 restatement of tests/update_ref.py: y, both losses, the TD errors,
EVERY critic and actor gradient and every entry of the four state_dicts, after
each of up to two SGD updates.  SGD's step is linear in the gradient, so the
parameters after it are as well conditioned as the gradients, and the second
update is still comparable (Adam's first step is lr * sign(g): it hides the
gradient's size, tests/test_trainer.py).

Bounds: update_ref.K, four times the float32 CPU trainer's own error against
the same restatement (tests/test_update_ref.py has the figures and the units:
u = 2^-24, a tensor in u max|ref|, a loss in u |ref|, a gradient tensor also in
relative L2; no floor, num_batches_tracked equal).

Cases (update_ref.LOSS_CASES) x trainers:
  batches   5 (no multiple of any tile), 16 (the goldens'), 62 and 65.  The
            fused MLP tail (train_ops.mlp_plan) is refused when m * n1 > 8192,
            m * n2 > 2048 or m > 256.  The actor's output branch is linear 2
            -> tanh (n1 = 2, n2 = 0): it is taken at every batch up to 256.
            The critic's is linear 128 -> leaky -> linear 1 (n1 = 128,
            n2 = 1): 64, the config's batch, is the last it takes
            (64 * 128 = 8192), and from 65 on the critic's head, the target's
            td_target and the actor loss's head fall back to torch.cat +
            library GEMMs.  No batch at or below 64 is on the far side, so 65
            is; 62 stands for the big batches inside (7936 of the 8192).  Why
            not 64 itself, and why these two run one update:
            tests/test_update_ref.py, "LeakyReLU's kink" -- the float64
            restatement's own gradients jump there under a float32-sized
            nudge of the observations, so no float32 update can be held to
            them (the kernel at m = 64, n1 = 128 is pinned in
            tests/test_gpu_mlp_tail.py).
  trainers  graph=False (host SGD, gradients in .grad) and graph=True,
            warmup=99 (DeviceSGD fed from _pending_grads: the eager twin of
            the captured graph), the default stream layout; one case with
            every stage on one stream (_fork -> None) at batch 16.
  losses    mse_loss unweighted; importance weights (test_is_weights'
            fixed_weights) with mse_loss and smooth_l1_loss at batch 16, where
            |y - q| falls on both sides of smooth-L1's knee
            (test_update_ref.test_smooth_l1_case_straddles_the_knee).
  rates     both learning rates times 2^-10, two updates (one where the
            kink test allows no second); one case at batch 16 runs the
            config's rates for one update.
Dropout stays at p = 0 (the folded dropout's mask is pinned at kernel level,
test_linear_dropout_folded_matches_f64).

The captured graph is not inspected here: the gradients are read from the
eager stages, and test_gpu_optim_device.test_trainer_graph_equals_eager_stages
carries the result over to graph mode bit for bit (float64 -> eager -> graph).

The worst figures on an MI355X, in units of u (printed by every case before
it asserts), with K beside them:
  y 7.1 (69), critic loss 7.5 (107), actor loss 159 (960), td 15.6 (188),
  critic gradients 141, relative L2 124 (1030, 660),
  actor gradients 167, relative L2 128 (1270, 1060),
  state 53.9 at the config's rates, 6.2 at the scaled ones (904).
The host and the device optimiser differ in the last digits of the losses
only; one stream equals two.  With the critic loss's gradient scaled by 1.001
every case fails (critic gradients 3.2e5 u, td 1390 u) while
test_update_matches_reference_gpu still passes.
"""
import pytest
import torch

import update_ref as R
from test_update_ref import assert_within, case_trainer, run_case

pytestmark = pytest.mark.gpu

TRAINERS = {'host_optimiser': dict(graph=False),
            'device_optimiser': dict(graph=True, warmup=99)}
CASES = [(case, kind, False) for case in R.LOSS_CASES for kind in TRAINERS]
CASES.append((R.LOSS_CASES[1], 'device_optimiser', True))


def _id(param):
    case, kind, one_stream = param
    return '%s-%s%s' % (R.case_id(case), kind, '-one_stream' if one_stream else '')


@pytest.mark.parametrize('param', CASES, ids=_id)
def test_update_against_float64(gpu, param):
    from aido1_amd import train_ops
    from aido1_amd.optim import DeviceStep
    case, kind, one_stream = param
    torch.backends.cudnn.allow_tf32 = False
    tr = case_trainer(case, gpu, **TRAINERS[kind])
    if one_stream:
        tr._fork = lambda: None
    device_step = kind == 'device_optimiser'
    assert isinstance(tr.critic_optim, DeviceStep) == device_step
    assert isinstance(tr.actor_optim, DeviceStep) == device_step
    # which side of the MLP tail's limit the critic's head is on (the actor's
    # is inside at every batch here)
    b = case[0]
    parts = [torch.zeros(b, 256, device=gpu), torch.zeros(b, 2, device=gpu)]
    assert (train_ops.mlp_plan(tr.critic.net.output_nets[0], parts) is not None) == (b <= 64)
    assert train_ops.mlp_plan(tr.actor.net.output_nets[0],
                              [torch.zeros(b, 512, device=gpu)]) is not None
    per_update, seen = run_case(case, tr, sync=torch.cuda.synchronize)
    # the device optimiser read the autograd outputs themselves, the host
    # optimiser .grad; every update ran the eager stages
    assert seen['critic_pending'] == device_step and seen['actor_pending'] == device_step
    assert tr._graphs is None
    tr.check()
    total = R.Worst()
    for worst in per_update:
        total.merge(worst)
    print(_id(param), 'units of u:', total)
    assert_within(total, R.K)
