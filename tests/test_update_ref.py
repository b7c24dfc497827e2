"""tests/update_ref.py, the float64 restatement of one DDPG update, checked on
the host, and the yardstick that sets the GPU bounds of
tests/test_gpu_update_grads.py.

1. The restatement with torch Adam reproduces the reference's own recorded
   float64 update (tests/golden/ddpg_update_f64.json, three updates) to the
   tolerances of test_trainer.test_update_matches_reference_f64_cpu: without
   this it would only be checked against aido1_amd/trainer.py.
2. It equals the float64 CPU trainer with SGD over two updates: gradients,
   losses, y, TD errors and every state_dict entry to 1e-10 of each tensor's
   largest magnitude.
3. The yardstick: the float32 CPU trainer (SGD, graph=False) against the
   restatement on the cases of update_ref.LOSS_CASES, in the units of
   update_ref.units / l2_units (u = 2^-24; a tensor in u max|ref|, a loss in
   u |ref|, a gradient tensor also as ||g - g64|| / ||g64|| in u; no floor).
4. Every case keeps clear of LeakyReLU's kink (below).

The bounds update_ref.K are 4 times the worst CPU float32 figure over the
cases at batches 5 and 16, all updates (the GPU sums in another order; the
rule and the margin of tests/test_gpu_bn_tail.py's K_Y, K_G).  Measured:
  y 17.2, critic loss 26.7, actor loss 240 (a mean of both signs), td 47,
  critic gradients 257 (relative L2 165), actor gradients 318 (L2 265),
  state after the update 226 (a critic running mean after one update at the
  config's learning rates; 30.1 with the scaled rates)
  -> K: y 69, critic_loss 107, actor_loss 960, td 188, critic_grad 1030,
     critic_grad_l2 660, actor_grad 1270, actor_grad_l2 1060, state 904.
A critic loss gradient scaled by 1.001 is 16 800 of these units.

The batches above 16 set no constant.  torch's CPU float32 kernels for
channels_last tensors lose precision with the batch (y: 12 u at batch 16,
120 u at 62, 85 u at 65; m = 70001 in tests/test_gpu_bn_tail.py is the same
finding), and with a forward that noisy some pre-activation changes sides of
LeakyReLU's kink, after which the gradients are off by 2 to 4e5 u at 62, 64 and
65 alike.  That would only loosen the bounds.  The GPU kernels' forward is
more accurate than either (y within 9 u at every batch), so the big batches
are held to the same K on the GPU; on the CPU their first update's critic
loss is held to K / 2 and the rest is printed.

LeakyReLU's kink.  The gradient is discontinuous in the inputs wherever a
pre-activation crosses zero, and the conv biases' and BatchNorm shifts'
gradients are cancelling sums, so one element of one layer taking the other
branch moves them by 1e4 to 1e5 u.  A float32 run takes the other branch
wherever |z| is below its own forward error, and then no bound of the form
above can hold for ANY float32 arithmetic.  Whether a case is exposed is a
property of the float64 restatement alone: multiply both observation batches
by 1 + 8 u (the size of a float32 forward error) and see how far its own
gradients move.  Every case must stay within K / 4 at every update it runs
(test_reference_gradients_survive_a_float32_sized_nudge; measured 33 to 95 u).
That, and nothing measured on the GPU, chose the big batches and the number
of updates:
  * the fused MLP tail's limit for the critic's head is m <= 64; no batch at
    or below the config's 64 lies beyond it, so 65 is the far side;
  * 64 moves by 1.8e5 u at its first update, 63 by 4.7e4 u; 62 moves by 92 u
    at the first update and 6.6e5 u at the second, 65 by 85 u and 6.5e4 u:
    62 (m * n1 = 7936 of the 8192 the kernel takes) and 65 run one update;
  * the smooth-L1 case moves by 4.3e4 u at its second update: one update.
"""
import numpy as np
import pytest

from conftest import golden
import update_ref as R
from update_ref import formula_batch
from formulas import param_summary  # noqa: E402  (update_ref put tests/golden on the path)


def case_trainer(case, device, double=False, **kw):
    """test_gpu_optim_device._trainer('sgd', device, ...) on the case's copy of
    the config (its learning rates), loss kind and weights switch."""
    from aido1_amd.actor import ConfigActor, ConfigCritic
    from aido1_amd.trainer import DDPGTrainer
    b, kind, weighted, scaled, updates = case
    cfg = R.case_config('sgd', scaled)
    actor = ConfigActor(R.no_dropout(cfg['model']['actor']))
    critic = ConfigCritic(R.no_dropout(cfg['model']['critic']))
    actor.load_state_dict(R.formula_state_dict(actor.state_dict()))
    critic.load_state_dict(R.formula_state_dict(critic.state_dict()))
    if double:
        actor.double()
        critic.double()
    tr = DDPGTrainer(cfg, actor, critic, device=device, importance_weights=weighted, **kw)
    tr.critic_loss_kind = kind
    return tr


def capture_grads(tr):
    """Wrap tr._opt_step: before each optimiser step, clone the gradients it
    is about to read -- the device optimiser's inputs (_pending_grads), or
    .grad where nothing is pending (the host optimiser; a device optimiser
    reading .grad).  -> the dict the clones land in, by network name, each a
    dict by parameter name.  Only eager stages pass through here: a captured
    graph is not inspected (test_trainer_graph_equals_eager_stages ties it to
    the eager stages bit for bit)."""
    seen = {}
    inner = tr._opt_step

    def wrapped(opt, module, *stages):
        grads = tr._pending_grads.get(id(module))
        name = 'actor' if module is tr.actor else 'critic'
        seen[name + '_pending'] = grads is not None
        if grads is None:
            grads = [p.grad for p in module.parameters()]
        seen[name] = {n: g.detach().clone() for (n, _), g in
                      zip(module.named_parameters(), grads)}
        return inner(opt, module, *stages)
    tr._opt_step = wrapped
    return seen


def run_case(case, tr, sync=None):
    """The case's updates on `tr` against the cached reference -> the worst
    figures (update_ref.Worst) per update, and the last update's captured
    gradients (capture_grads)."""
    seen = capture_grads(tr)
    batch, w = formula_batch(case[0]), R.case_weights(case)
    ref = R.reference(case)
    out = []
    for k in range(R.case_updates(case)):
        seen.clear()
        metrics, info = tr.update(batch, **({'weights': w} if case[2] else {}))
        if sync is not None:
            sync()
        worst = R.Worst()
        R.measure(worst, ref[k], tr._y, metrics['critic_loss'].double() ** 2,
                  metrics['actor_loss'], info['td_error'], seen['critic'], seen['actor'],
                  {n: getattr(tr, n).state_dict() for n in R.NETS}, tag='u%d ' % (k + 1))
        out.append(worst)
    return out, seen


def assert_within(worst, bounds, divide=1.0):
    bad = {k: v for k, (v, _) in worst.fig.items() if not v <= bounds[k] / divide}
    assert not bad, 'beyond the bound: %s; all: %s' % (bad, worst)


# ---- 1. against the reference's own recorded update ---------------------------------------
def test_restatement_reproduces_the_recorded_update():
    cfg = R.case_config('adam', scaled=False)
    outs, nets = R.run_reference(cfg, formula_batch(16), 3)
    ref = golden('ddpg_update_f64.json')
    rtol, atol = 1e-8, 1e-9
    for k, o in enumerate(outs):
        np.testing.assert_allclose(float(o['critic_loss'].sqrt()), ref['critic_loss'][k], rtol=rtol)
        np.testing.assert_allclose(float(o['actor_loss']), ref['actor_loss'][k], rtol=rtol)
        np.testing.assert_allclose(o['td'].numpy().reshape(-1), ref['td_error'][k],
                                   rtol=rtol, atol=atol)
    for name in R.NETS:
        got = param_summary(nets[name])
        assert list(got) == list(ref[name]), name
        for key, vals in ref[name].items():
            # test_trainer.check_against_reference's exceptions: the conv
            # biases and the running means that carry them
            a_ = 1e-5 if key.endswith(('kernel.bias', 'running_mean')) else atol
            np.testing.assert_allclose(got[key], vals, rtol=rtol, atol=a_, err_msg=name + key)


# ---- 2. against the float64 CPU trainer ---------------------------------------------------
@pytest.mark.parametrize('case', [(16, 'mse_loss', False, True, 2),
                                  (16, 'smooth_l1_loss', True, True, 2)], ids=R.case_id)
def test_restatement_equals_the_float64_trainer(case):
    """SGD, two updates, the scaled learning rates; the trainer's gradients
    read from .grad (graph=False).  Every figure within 1e-10 of its tensor's
    largest magnitude, i.e. 1e-10 / u units."""
    assert R.case_updates(case) == 2
    tr = case_trainer(case, 'cpu', double=True, graph=False)
    for worst in run_case(case, tr)[0]:
        print(R.case_id(case), 'float64 trainer, units of u:', worst)
        assert_within(worst, {k: 1e-10 / R.U for k in R.KINDS_OF_FIGURE})


def test_smooth_l1_case_straddles_the_knee():
    """Some |y - q| of the smooth-L1 case on each side of 1 (both arms of the
    loss and of its gradient)."""
    for o in R.reference(R.LOSS_CASES[6]):
        d = o['d0'].abs()
        assert bool((d < 1.0).any()) and bool((d > 1.0).any()), d.reshape(-1)


# ---- 3. the yardstick ---------------------------------------------------------------------
SMALL = [c for c in R.LOSS_CASES if c[0] <= 16]
BIG = [c for c in R.LOSS_CASES if c[0] > 16]


@pytest.mark.parametrize('case', SMALL, ids=R.case_id)
def test_cpu_float32_is_within_half_the_bounds(case):
    """The float32 CPU trainer in the bounds' units (the module docstring has
    the figures): the K are 4 times the worst of them, and this asserts K / 2,
    so that another build of torch summing in another order does not fail."""
    tr = case_trainer(case, 'cpu', graph=False)
    for worst in run_case(case, tr)[0]:
        print(R.case_id(case), 'CPU float32, units of u:', worst)
        assert_within(worst, R.K, divide=2.0)


@pytest.mark.parametrize('case', BIG, ids=R.case_id)
def test_cpu_float32_at_the_big_batches(case):
    """The same measurement at the batches that set no constant (module
    docstring): the first update's critic loss, which no LeakyReLU derivative
    enters, is held to K / 2 here as well; the rest is printed."""
    tr = case_trainer(case, 'cpu', graph=False)
    worst = run_case(case, tr)[0][0]
    print(R.case_id(case), 'CPU float32, units of u:', worst)
    assert worst.fig['critic_loss'][0] <= R.K['critic_loss'] / 2


# ---- 4. the cases stay clear of LeakyReLU's kink ------------------------------------------
@pytest.mark.parametrize('case', R.LOSS_CASES, ids=R.case_id)
def test_reference_gradients_survive_a_float32_sized_nudge(case):
    """Every gradient of the float64 restatement, at every update of every
    case, moves by at most K / 4 when both observation batches are multiplied
    by 1 + 8 u (module docstring, "LeakyReLU's kink"): the condition under
    which a float32 update can be held to it at all."""
    base, nudged = R.reference(case), R.nudged_reference(case)
    worst = R.Worst()
    for k, (a, b) in enumerate(zip(base, nudged)):
        for net in ('critic', 'actor'):
            for name, g in a[net + '_grads'].items():
                tag = 'u%d %s' % (k + 1, name)
                worst.add(net + '_grad', R.units(b[net + '_grads'][name], g), tag)
                worst.add(net + '_grad_l2', R.l2_units(b[net + '_grads'][name], g), tag)
    print(R.case_id(case), 'nudged reference, units of u:', worst)
    for kind in R.GRAD_FIGURES:
        assert worst.fig[kind][0] <= R.K[kind] / 4, (kind, worst.fig[kind])
