"""DDPG update and the full training loop on the GPU.

The update is compared with the reference's own DDPGTrainer.update
(tests/golden/ddpg_update.json, run on CPU in float32).  Tolerance: the GPU
convolutions (MIOpen) sum in a different order than CPU ones, so losses and
TD errors agree to ~1e-5 relative; parameters after three Adam steps agree to
rtol 1e-3 / atol 1e-3 (Adam's first steps move each weight by ~lr * sign(g),
so a gradient within rounding noise of zero may step the other way).
Adam hides a gradient's magnitude: tests/test_gpu_update_grads.py holds every
gradient of the eager GPU stages to a float64 restatement with SGD."""
import pytest
import torch

from conftest import golden
from test_trainer import check_against_reference, formula_batch, make_trainer

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('graph', [False, True])
def test_update_matches_reference_gpu(gpu, graph):
    """graph=True: update 1 eager, updates 2-3 replay the captured HIP graph."""
    torch.backends.cudnn.allow_tf32 = False
    tr = make_trainer(gpu, graph=graph, warmup=1)
    check_against_reference(tr, formula_batch(16), rtol=1e-3, atol=1e-3)
    if graph:
        assert tr._graphs is not None and len(tr._graphs) == 1


@pytest.mark.parametrize('prioritized,graph,size', [(True, True, 1000), (False, False, 1000),
                                                     (True, True, 1024)])
def test_train_loop_runs(gpu, prioritized, graph, size):
    """size 1024 = 8 decisions of 128 envs: the frame store (replay.py)."""
    from aido1_amd.train_loop import TrainLoop
    cfg = golden('reference_config.json')
    loop = TrainLoop(cfg, n_envs=128, device=0, seed=5, buffer_size=size, batch_size=32,
                     prioritized=prioritized, graph=graph)
    assert (loop.replay.frame_envs is not None) == (size == 1024)
    w0 = loop.trainer.actor.net.input_nets[0].internal_modules[0].kernel.weight.detach().clone()
    t0 = loop.rollout.actor.w[1].detach().clone()
    loop.reset()
    for _ in range(12):
        loop.step()
    # the guards name the first stage that produced NaN / Inf (and the
    # replay's rejected priorities), before any assertion on the results
    try:
        rec = loop.check()
    except Exception:
        from test_gpu_guard import _report_rollout_state
        _report_rollout_state(loop)
        raise
    assert rec['tick'] == 12
    assert len(loop.replay) == size and loop.updates == 12 and loop.decisions == 12
    assert torch.isfinite(loop.metrics['critic_loss']) and torch.isfinite(loop.metrics['actor_loss'])
    w1 = loop.trainer.actor.net.input_nets[0].internal_modules[0].kernel.weight
    assert not torch.equal(w0, w1)
    # the exploring envs act with the online actor, the exploiters with the
    # target actor (train_loop._refresh)
    assert not torch.equal(t0, loop.rollout.actor.w[1])
    for mine, src in ((loop.rollout.actor, loop.trainer.actor),
                      (loop.rollout.exploit_actor, loop.trainer.target_actor)):
        k = src.net.input_nets[0].internal_modules[0].kernel.weight
        assert torch.equal(mine.w[0].float(), k.detach().to(mine.w[0].dtype).float())
    st = loop.replay.storage
    if size == 1024:
        obs, act, rew, nxt, done = loop.replay._encode_sample(torch.arange(size, device=gpu))
        p = loop.replay._next_idx          # 12 decisions of 128 rows: 512
        assert p == 512
        # the last decision's next_obs is the rollout's current stack
        assert torch.equal(nxt[p - 128:p], loop.rollout.stack())
        # obs of a decision = next_obs of the env's previous decision
        assert torch.equal(obs[p - 128:p], nxt[p - 256:p - 128])
        assert obs.shape == (size, 3, 120, 160) and st['action'].shape == (size, 2)
    else:
        assert st['obs'].shape == (1000, 3, 120, 160) and st['action'].shape == (1000, 2)
    assert float(st['action'].min()) >= 0.0                  # mapped a/2 + 0.5 stored
    if prioritized:
        loop.replay.check()
        _, _, mp = loop.replay.trees()
        assert mp.item() >= 1.0
    assert loop.rollout.stats()['decisions'] == 128 * 12


@pytest.mark.parametrize('graph', [False, True])
def test_two_stream_stages_equal_one_stream(gpu, graph):
    """The update's side-stream branches (trainer._fork: the targets' forward
    beside the critic's, the stepped critic's trunk beside the actor's
    forward, the TD forward beside the actor step and soft updates) against
    the same update with every stage on one stream: losses, TD errors and
    every state_dict entry (weights, BatchNorm running statistics) bit for
    bit over three updates, eager and captured as HIP graphs (two graph
    branches vs a chain).  Holds because no BatchNorm module is forwarded on
    both branches (its kernels' scratch is per module, train_ops)."""
    torch.backends.cudnn.allow_tf32 = False
    two = make_trainer(gpu, graph=graph, warmup=1)
    one = make_trainer(gpu, graph=graph, warmup=1)
    one._fork = lambda: None
    batch = formula_batch(16)
    for _ in range(3):
        m2, i2 = two.update(batch)
        m1, i1 = one.update(batch)
        torch.cuda.synchronize()
        for k in ('critic_loss', 'actor_loss'):
            assert torch.equal(m1[k], m2[k]), k
        assert torch.equal(i1['td_error'], i2['td_error'])
    for a, b in ((two.actor, one.actor), (two.critic, one.critic),
                 (two.target_actor, one.target_actor), (two.target_critic, one.target_critic)):
        sa, sb = a.state_dict(), b.state_dict()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
    if graph:
        assert two._graphs is not None and one._graphs is not None


# ---- the drop pool (train_ops.drop_pool) around the stages ---------------------------------
def _keep_dropout(monkeypatch):
    """make_trainer with config.json's dropouts left in (it zeroes them for
    the golden runs, and with p = 0 no site folds and no pool is opened)."""
    import test_trainer
    monkeypatch.setattr(test_trainer, 'no_dropout', lambda net_config: net_config)


@pytest.mark.parametrize('dropout', [False, True])
def test_failed_update_releases_drop_pool(gpu, monkeypatch, dropout):
    """An eager update that raises between _stage_critic (which opens the
    pool) and the end of _stage_targets leaves no pool behind: _DROP is back
    at its idle state, and three seeded updates of a trainer built afterwards
    equal, bit for bit, those of one built after _DROP was reset by hand.
    The failure is a host RuntimeError from a replaced _stage_actor."""
    from aido1_amd import train_ops
    torch.backends.cudnn.allow_tf32 = False
    if dropout:
        _keep_dropout(monkeypatch)
    batch = formula_batch(16)
    bad = make_trainer(gpu)

    def fail():
        raise RuntimeError('stage failed')
    bad._stage_actor = fail
    with pytest.raises(RuntimeError, match='stage failed'):
        bad.update(batch)
    assert train_ops._DROP['pool'] is None and train_ops._DROP['next'] == 0
    # with dropouts the pool was open when the stage failed (the critic stage's sites)
    assert (bad.drop_sites_used > 0) == dropout

    def three_updates():
        torch.manual_seed(7)
        tr = make_trainer(gpu)
        tds = [tr.update(batch)[1]['td_error'].clone() for _ in range(3)]
        torch.cuda.synchronize()
        return tr, tds
    after, td_after = three_updates()
    train_ops._DROP.update(pool=None, next=0)
    control, td_control = three_updates()
    for a, b in zip(td_after, td_control):
        assert torch.equal(a, b)
    for name in ('actor', 'critic', 'target_actor', 'target_critic'):
        sa, sb = getattr(after, name).state_dict(), getattr(control, name).state_dict()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (name, k)


@pytest.mark.parametrize('dropout', [False, True])
@pytest.mark.parametrize('layout', ['default', 'split_target', 'importance_weights',
                                    'one_stream'])
def test_update_consumes_its_drop_sites(gpu, monkeypatch, layout, dropout):
    """One eager update takes exactly DDPGTrainer.DROP_SITES slices of the
    pool in every stage layout: none drawn past its end, none wasted.
    make_trainer's own networks (dropout p = 0) fold nothing, so no pool is
    opened and the count is 0."""
    from aido1_amd import train_ops
    if dropout:
        _keep_dropout(monkeypatch)
    tr = make_trainer(gpu, importance_weights=layout == 'importance_weights')
    tr.split_target = layout == 'split_target'
    tr.multi_stream = layout != 'one_stream'
    tr.update(formula_batch(16))
    torch.cuda.synchronize()
    assert tr.drop_sites_used == (tr.DROP_SITES if dropout else 0)
    assert train_ops._DROP['pool'] is None and train_ops._DROP['next'] == 0


def test_no_pool_without_fold_dropout(gpu, monkeypatch):
    """fold_dropout=False (the A/B switch): the dropouts stay torch's, no pool
    is opened."""
    from aido1_amd import train_ops
    _keep_dropout(monkeypatch)
    tr = make_trainer(gpu)
    tr.fold_dropout = False
    drawn = []
    monkeypatch.setattr(train_ops, 'drop_pool', lambda *a, **k: drawn.append(a))
    try:
        tr.update(formula_batch(16))
        torch.cuda.synchronize()
    finally:
        train_ops.FOLD_DROPOUT = True       # the global the trainer set (its default)
    assert not drawn and tr.drop_sites_used == 0
