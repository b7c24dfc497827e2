"""Importance weights of the prioritized replay in the critic loss, on the GPU:
dt_loss_w / dt_loss_w_bwd (train_ops.weighted_loss) against float64 torch and
against the unweighted kernels bit for bit, dt_frame_gather_w
(replay.gather_into), DDPGTrainer(importance_weights=True) captured against
eager and against the CPU in float64, TrainLoop(importance_weights=True) and
the guard.  The CPU side is tests/test_is_weights.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_is_weights import KINDS, fixed_weights, kind_trainer
from test_trainer import formula_batch, make_trainer

pytestmark = pytest.mark.gpu

NETS = ('actor', 'critic', 'target_actor', 'target_critic')


def _ref_loss(a, b, w, kind):
    terms = (a - b) ** 2 if kind == 'mse_loss' else F.smooth_l1_loss(a, b, reduction='none')
    return (w * terms).mean()


# ---- 1. the kernels ------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('m', [1, 63, 64, 65, 255, 256, 257, 300])   # wave and workgroup edges
def test_weighted_loss_kernels_match_float64(gpu, m, kind):
    """dt_loss_w / dt_loss_w_bwd through train_ops.weighted_loss against the
    float64 torch expression on the same float32 inputs, upstream gradient
    0.5; smooth-L1 with the branch edges d = +-1, 0 and nextafter(1, 0) forced
    in.  test_fused_losses_match_torch's bounds (float32 terms, float64 sum)."""
    from aido1_amd import train_ops
    g = torch.Generator(device=gpu).manual_seed(1000 + m)
    a = 2 * torch.randn(m, 1, device=gpu, generator=g)
    b = torch.randn(m, 1, device=gpu, generator=g)
    w = 0.001 + 0.999 * torch.rand(m, 1, device=gpu, generator=g)
    if m > 2:
        w[m // 2] = 0.0
    if kind == 'smooth_l1_loss' and m >= 4:
        one = torch.ones((), device=gpu)
        below = torch.nextafter(one, 0 * one)              # the last float32 of the quadratic arm
        a[:4, 0] = torch.stack([3 * one, 0 * one, 0.75 * one, below])
        b[:4, 0] = torch.stack([2 * one, one, 0.75 * one, 0 * one])     # d = +1, -1, 0, below
        assert (a - b)[:4, 0].tolist() == [1.0, -1.0, 0.0, below.item()]
    a.requires_grad_(True)
    loss = train_ops.weighted_loss(a, b, w, kind)
    assert type(loss.grad_fn).__name__ == '_LossWBackward'
    a64 = a.detach().double().requires_grad_(True)
    ref = _ref_loss(a64, b.double(), w.double(), kind)
    torch.testing.assert_close(loss.double(), ref, rtol=1e-6, atol=1e-7)
    loss.backward(torch.tensor(0.5, device=gpu))
    ref.backward(torch.tensor(0.5, dtype=torch.float64, device=gpu))
    torch.testing.assert_close(a.grad.double(), a64.grad, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize('m', [1, 64, 300])
def test_weighted_loss_bit_identities(gpu, m):
    """Ones equal w = NULL for both kinds, forward and backward; kind 0 with
    ones is train_ops.mse_loss (dt_loss kind 0) and its gradient; all bit for
    bit.  [m, 1] against w [m] broadcasts in torch and is not the kernel's."""
    from aido1_amd import train_ops
    g = torch.Generator(device=gpu).manual_seed(2000 + m)
    a0 = 2 * torch.randn(m, 1, device=gpu, generator=g)
    b = torch.randn(m, 1, device=gpu, generator=g)
    up = torch.tensor(0.5, device=gpu)

    def run(fn):
        a = a0.clone().requires_grad_(True)
        loss = fn(a)
        loss.backward(up)
        return loss.detach(), a.grad
    ones = torch.ones(m, 1, device=gpu)
    for kind in KINDS:
        l1, g1 = run(lambda a: train_ops.weighted_loss(a, b, ones, kind))
        l0, g0 = run(lambda a: train_ops.weighted_loss(a, b, None, kind))
        assert torch.equal(l1, l0) and torch.equal(g1, g0), kind
    lw, gw = run(lambda a: train_ops.weighted_loss(a, b, ones, 'mse_loss'))
    lm, gm = run(lambda a: train_ops.mse_loss(a, b))
    assert torch.equal(lw, lm) and torch.equal(gw, gm)
    # w of shape [m] broadcasts to [m, m]: the torch expression, not the kernel
    w1 = 0.5 + 0.5 * torch.rand(m, device=gpu, generator=g)
    a = a0.clone().requires_grad_(True)
    for kind in KINDS:
        loss = train_ops.weighted_loss(a, b, w1, kind)
        assert type(loss.grad_fn).__name__ == 'MeanBackward0'
        torch.testing.assert_close(loss, _ref_loss(a, b, w1, kind))


# ---- 2. the gather -------------------------------------------------------------------------
@pytest.mark.parametrize('index', [False, True])
def test_frame_gather_w(gpu, index):
    """dt_frame_gather_w: out['w'] is the float32 of the sampled float64
    weights by batch position, every other key what gather_into writes without
    weights; the stacked storage (torch copies) gives the same 'w'."""
    from test_replay import _frame_steps
    from aido1_amd.replay import PrioritizedReplayBuffer
    g = torch.Generator().manual_seed(4)
    n, size = 256, 1024
    a = PrioritizedReplayBuffer(size, 0.6, device=gpu, frame_envs=n)
    b = PrioritizedReplayBuffer(size, 0.6, device=gpu)
    for _ in _frame_steps(a, b, n, 7, g, index=index):
        pass
    shape = (3,) + tuple(a.frames.shape[1:])

    def outputs(batch, with_w):
        z = lambda *s: torch.full(s, -7.0, device=gpu)
        out = {'obs': z(batch, *shape).contiguous(memory_format=torch.channels_last),
               'nxt': z(batch, *shape).contiguous(memory_format=torch.channels_last),
               'act': z(batch, 2), 'rew': z(batch, 1), 'notdone': z(batch, 1)}
        if with_w:
            out['w'] = z(batch, 1)
        return out
    for batch in (1, 5, 64):
        u = torch.rand(batch, generator=g, dtype=torch.float64)
        idx, weights = a.sample_indices(batch, 0.4, u=u)
        idx_b, weights_b = b.sample_indices(batch, 0.4, u=u)
        assert torch.equal(idx, idx_b) and torch.equal(weights, weights_b)
        assert weights.dtype == torch.float64
        want = a.gather_into(idx, outputs(batch, False))
        assert 'w' not in want
        for buf in (a, b):
            got = buf.gather_into(idx, outputs(batch, True), weights=weights)
            assert torch.equal(got['w'], weights.float().reshape(-1, 1))
            for k in want:
                assert torch.equal(got[k], want[k]), k
        # weights without a 'w' to write them into change nothing
        got = a.gather_into(idx, outputs(batch, False), weights=weights)
        assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)


# ---- 3. the trainer ------------------------------------------------------------------------
def _rotated(k):
    return np.roll(fixed_weights(), k).astype(np.float32)


def _same(pairs, tr_a, tr_b):
    for x, y in pairs:
        assert torch.equal(x, y)
    for name in NETS:
        sa, sb = getattr(tr_a, name).state_dict(), getattr(tr_b, name).state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), name + ' ' + k


@pytest.mark.parametrize('kind', KINDS)
def test_weighted_graph_equals_eager_stages(gpu, kind):
    """warmup=1 (updates 2-4 replay the one captured graph) against warmup=99
    (the same stages run eagerly), the weights another rotation of the fixed
    vector every update: a graph that baked the first weights in, or whose 'w'
    was not refilled, differs.  Bit for bit."""
    torch.backends.cudnn.allow_tf32 = False
    cap = kind_trainer(gpu, kind, graph=True, warmup=1, importance_weights=True)
    eag = kind_trainer(gpu, kind, graph=True, warmup=99, importance_weights=True)
    batch = formula_batch(16)
    pairs = []
    for k in range(4):
        m1, i1 = cap.update(batch, weights=_rotated(k))
        m2, i2 = eag.update(batch, weights=_rotated(k))
        torch.cuda.synchronize()
        assert torch.equal(cap._in['w'].reshape(-1).cpu(), torch.from_numpy(_rotated(k)))
        pairs += [(m1[key].clone(), m2[key].clone()) for key in ('critic_loss', 'actor_loss')]
        pairs.append((i1['td_error'].clone(), i2['td_error'].clone()))
    assert cap._graphs is not None and len(cap._graphs) == 1 and eag._graphs is None
    assert 'w' in cap.static_inputs(16)
    _same(pairs, cap, eag)
    cap.check()


@pytest.mark.parametrize('warmup', [99, 1])            # eager stages, captured graph
def test_ones_equal_the_unweighted_trainer(gpu, warmup):
    """mse_loss with weights of ones against a trainer built without the
    switch (dt_loss / dt_loss_bwd): losses, TD errors and every state_dict
    entry bit for bit over 3 updates -- the kernels' rounding order end to
    end."""
    torch.backends.cudnn.allow_tf32 = False
    wtd = make_trainer(gpu, graph=True, warmup=warmup, importance_weights=True)
    ref = make_trainer(gpu, graph=True, warmup=warmup)
    batch = formula_batch(16)
    pairs = []
    for _ in range(3):
        m1, i1 = wtd.update(batch, weights=np.ones(16))
        m2, i2 = ref.update(batch)
        torch.cuda.synchronize()
        pairs += [(m1[key].clone(), m2[key].clone()) for key in ('critic_loss', 'actor_loss')]
        pairs.append((i1['td_error'].clone(), i2['td_error'].clone()))
    assert 'w' not in ref.static_inputs(16)
    assert (wtd._graphs is not None) == (warmup == 1) == (ref._graphs is not None)
    _same(pairs, wtd, ref)


@pytest.mark.parametrize('kind', KINDS)
def test_weighted_first_update_against_cpu_float64(gpu, kind):
    """The first weighted update in float32 on the GPU against float64 on the
    CPU (test_update_matches_reference_gpu's bound for update 1; later float32
    updates are chaotic, tests/test_trainer.py)."""
    torch.backends.cudnn.allow_tf32 = False
    batch, w = formula_batch(16), fixed_weights()
    tr = kind_trainer(gpu, kind, graph=True, warmup=1, importance_weights=True)
    ref = kind_trainer('cpu', kind, double=True, importance_weights=True)
    m, info = tr.update(batch, weights=w)
    rm, rinfo = ref.update(batch, weights=w)
    for key in ('critic_loss', 'actor_loss'):
        np.testing.assert_allclose(m[key].item(), rm[key].item(), rtol=1e-3, atol=1e-3,
                                   err_msg=key)
    np.testing.assert_allclose(info['td_error'].cpu().numpy(), rinfo['td_error'].numpy(),
                               rtol=1e-3, atol=1e-3)
    tr.check()


def test_nonfinite_weight_is_reported_as_batch(gpu):
    """'w' is part of the 'batch' guard scan: an inf among the weights is named
    by check()."""
    from aido1_amd.guard import NonFiniteError
    tr = make_trainer(gpu, importance_weights=True)
    w = fixed_weights()
    tr.update(formula_batch(16), weights=w)
    tr.check()
    w[3] = np.inf
    tr.update(formula_batch(16), weights=w)
    with pytest.raises(NonFiniteError, match='batch'):
        tr.check()


# ---- 4. the training loop ------------------------------------------------------------------
@pytest.mark.parametrize('size', [1024, 1000])          # the frame store, the stacked storage
def test_train_loop_importance_weights(gpu, size):
    """TrainLoop(importance_weights=True): the weights the sampler returned
    for the last update are the trainer's 'w' (their float32), all in (0, 1];
    beta follows beta_decay and is capped at 1."""
    from conftest import golden
    from aido1_amd.train_loop import TrainLoop
    decay = {'type': 'linear', 'args': {'initial_value': 0.4, 'final_value': 1.0, 'max_step': 10}}
    loop = TrainLoop(golden('reference_config.json'), n_envs=128, device=0, seed=5,
                     buffer_size=size, batch_size=32, graph=True, importance_weights=True,
                     beta_decay=decay)
    assert (loop.replay.frame_envs is not None) == (size == 1024)
    seen = []
    inner = loop.replay.sample_indices

    def recording(batch_size, beta=0.5, u=None):
        idx, w = inner(batch_size, beta, u)
        seen.append((beta, w.clone()))
        return idx, w
    loop.replay.sample_indices = recording
    loop.reset()
    for _ in range(12):
        loop.step()
    rec = loop.check()
    assert rec['tick'] == 12 and loop.updates == 12 and len(seen) == 12
    assert torch.isfinite(loop.metrics['critic_loss']) and torch.isfinite(loop.metrics['actor_loss'])
    assert loop.trainer._graphs is not None and len(loop.trainer._graphs) == 1
    betas = [b for b, _ in seen]
    assert betas[0] == pytest.approx(0.4) and betas[5] == pytest.approx(0.7) and betas[-1] == 1.0
    assert all(x <= y for x, y in zip(betas, betas[1:]))
    last = seen[-1][1]
    assert last.dtype == torch.float64
    assert torch.equal(loop.trainer.static_inputs(32)['w'], last.float().reshape(-1, 1))
    for _, w in seen:
        assert bool((w > 0).all()) and bool((w <= 1).all())


def test_train_loop_switches(gpu):
    from conftest import golden
    from aido1_amd.train_loop import TrainLoop
    cfg = golden('reference_config.json')
    with pytest.raises(ValueError):
        TrainLoop(cfg, n_envs=128, device=0, seed=5, buffer_size=1024, batch_size=32,
                  prioritized=False, importance_weights=True)
    loop = TrainLoop(cfg, n_envs=128, device=0, seed=5, buffer_size=1024, batch_size=32)
    assert 'w' not in loop.trainer.static_inputs(32)
    assert loop.trainer.importance_weights is False
    assert loop.beta_at(0) == loop.beta_at(10 ** 6) == cfg['training']['beta']
