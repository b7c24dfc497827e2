"""The device steps of the reference's other two optimisers (include/dttrain.h
dt_adamw / dt_sgd; aido1_amd/optim.py DeviceAdamW / DeviceSGD) on the GPU: the
chunk edges of the multi-tensor table, one step against the float64 formulas,
HIP-graph replay, load_state_dict to and from the host classes, the in-kernel
guards, and the trainer / training loop in graph mode with them.

The float64 bounds (test_one_step_against_float64) are |err| <= k u S per
element, u = 2^-24, S the float64 sum of the magnitudes of the terms that form
the value, k the number of float32 roundings on its path, counted from the
kernels (aido1_amd/csrc/dttrain.hip adamw_kernel / sgd_kernel; constants that
are rounded to float32 once count as one rounding each):

  AdamW  exp_avg     c = c*b1 + ob1*g          b1, c*b1, ob1, ob1*g, +          k = 5
                     S = |c| b1 + (1 - b1) |g|
         exp_avg_sq  d = d*b2 + (ob2*g)*g      b2, d*b2, ob2, ob2*g, *g, +      k = 6
                     S = d b2 + (1 - b2) g^2
         param       a = a - ss*(c/den); a = a - a*decay, den = sqrt(d) + eps:
                     the 5 of c, the 6 of d, sqrt, eps, + eps, /, ss, ss*q, -,
                     decay, a*decay, -                                           k = 21
                     S = |a| + ss S_c / den + |a'| lr wd   (a' the stepped a)
                     (d's roundings reach den halved by the root, which pays
                     for the second-order terms of (1 + u)^21)
  SGD    buffer      g' = g + wd*a; c = c*mom + g'   wd, wd*a, +, mom, c*mom, +  k = 6
                     S = |c| mom + |g| + wd |a|
         param       a = a - lr*c                    the 6 of c, lr, lr*c, -     k = 9
                     S = |a| + lr S_c
sqrt and the division are correctly rounded (the library is not built with
fast-math), no product is contracted into an add (-ffp-contract=off).
The kernels' own worst |err| / (u S) on an MI355X (printed before the
assertion): AdamW 1.86 / 2.00 / 2.12, SGD 2.03 / 1.26."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import golden
from test_trainer import formula_batch, formula_state_dict, no_dropout, param_summary

pytestmark = pytest.mark.gpu

KINDS = ['adamw', 'sgd']
U = 2.0 ** -24
B1, B2, EPS, WD, MOM = 0.9, 0.999, 1e-8, 1e-4, 0.9
NAN = float('nan')


def _device(kind, params, gpu):
    from aido1_amd.optim import DeviceAdamW, DeviceSGD, make_optimizer
    opt = make_optimizer(kind, params, capturable=True, device=gpu)
    assert type(opt) is (DeviceAdamW if kind == 'adamw' else DeviceSGD)
    return opt


def _host(kind, params):
    """optim.AdamW / torch.optim.SGD with the reference's hyper-parameters."""
    from aido1_amd.optim import make_optimizer
    return make_optimizer(kind, params)


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = torch.empty_like(p)
        p.grad.copy_(g)


def _assert_close_state(kind, opt, params, ropt, ref):
    """The tolerances of test_adam_at_chunk_edges (tests/test_gpu_bn_tail.py)."""
    for p, q in zip(params, ref):
        torch.testing.assert_close(p, q, rtol=1e-6, atol=1e-7)
        st, rst = opt.state[p], ropt.state[q]
        if kind == 'adamw':
            torch.testing.assert_close(st['exp_avg'], rst['exp_avg'], rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(st['exp_avg_sq'], rst['exp_avg_sq'], rtol=1e-6, atol=1e-10)
        else:
            torch.testing.assert_close(st['momentum_buffer'], rst['momentum_buffer'],
                                       rtol=1e-5, atol=1e-6)


def _assert_same_state(opt_a, params_a, opt_b, params_b):
    for p, q in zip(params_a, params_b):
        assert torch.equal(p, q)
        for k in opt_a.STATE:
            assert torch.equal(opt_a.state[p][k], opt_b.state[q][k]), k


# ---- 1. the chunk edges (DT_MT_CHUNK = 4096) -----------------------------------------------
MT_SIZES = [1, 255, 256, 4095, 4096, 4097, 8192, 12289]
SENTINEL = 12345.0


def _carve(dev, sizes, fill):
    """One flat tensor per size out of a single buffer with a sentinel element
    after each; fill(n) gives a tensor's content.  -> (views, buffer, mask of
    the sentinels)."""
    buf = torch.full((sum(sizes) + len(sizes),), SENTINEL, device=dev)
    mask = torch.ones_like(buf, dtype=torch.bool)
    views, at = [], 0
    for n in sizes:
        buf[at:at + n] = fill(n)
        mask[at:at + n] = False
        views.append(buf[at:at + n])
        at += n + 1
    return views, buf, mask


@pytest.mark.parametrize('kind', KINDS)
def test_chunk_edges(gpu, kind):
    """One device optimiser over flat parameters of 1 ... 12289 elements (one
    workgroup a chunk of 4096, partial and exact last chunks), three steps with
    a changing lr against the eager optimiser of the same kind; the element
    after each parameter's, gradient's and state tensor's storage is not
    written, the counter is left at zero."""
    torch.manual_seed(31)
    zeros = lambda n: torch.zeros(n, device=gpu)
    pv, pbuf, pmask = _carve(gpu, MT_SIZES, lambda n: torch.randn(n, device=gpu))
    gv, gbuf, gmask = _carve(gpu, MT_SIZES, zeros)
    params = [nn.Parameter(v) for v in pv]
    ref = [nn.Parameter(v.detach().clone()) for v in pv]
    opt = _device(kind, params, gpu)
    bufs = [(pbuf, pmask), (gbuf, gmask)]
    for k in opt.STATE:
        sv, sbuf, smask = _carve(gpu, MT_SIZES, zeros)
        bufs.append((sbuf, smask))
        for p, s in zip(params, sv):
            opt.state[p][k] = s
    for p, g in zip(params, gv):
        p.grad = g
    ropt = _host(kind, ref)
    for k in range(3):
        lr = 1e-3 * (1.0 - 0.1 * k)
        opt.param_groups[0]['lr'].fill_(lr)
        ropt.param_groups[0]['lr'] = lr
        for p, q in zip(params, ref):
            g = torch.randn_like(p) * (0.1 + k)
            p.grad.copy_(g)
            q.grad = g.clone()
        opt.step()
        ropt.step()
    assert opt._table is not None and opt._table.n_chunks == 13
    _assert_close_state(kind, opt, params, ropt, ref)
    assert int(opt._counter) == 0
    if kind == 'adamw':
        assert float(opt._step_t) == 3.0
        assert all(float(opt.state[p]['step']) == 3.0 for p in params)
    for buf, mask in bufs:
        assert bool((buf[mask] == SENTINEL).all())


# ---- 2. one step against the float64 formulas ----------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_one_step_against_float64(gpu, kind):
    """One device step from a float32 state (non-zero moments / buffers, step
    count 7) on a conv (channels_last) + BatchNorm + linear stack against the
    float64 evaluation of include/dttrain.h's formulas from the same float32
    state, per element within k u S (module docstring: AdamW k = 5 / 6 / 21 for
    exp_avg / exp_avg_sq / the parameter, SGD k = 6 / 9 for the buffer / the
    parameter; no floor).  The BatchNorm bias has an exactly zero gradient on
    a zero state (what materialize_grads hands an unused parameter): AdamW
    leaves p - p * float32(lr * wd) exactly and the moments at 0, SGD takes the
    weight-decay-only step exactly."""
    torch.manual_seed(32)
    net = nn.Sequential(nn.Conv2d(3, 32, 8, stride=2), nn.BatchNorm2d(32), nn.Flatten(),
                        nn.Linear(32 * 3 * 3, 5)).to(gpu).to(memory_format=torch.channels_last)
    params = list(net.parameters())
    unused = net[1].bias
    with torch.no_grad():
        unused.uniform_(-1, 1)
    opt = _device(kind, params, gpu)
    lr = 7.3e-4
    opt.param_groups[0]['lr'].fill_(lr)
    grads = []
    for p in params:
        zero = p is unused
        grads.append(torch.zeros_like(p) if zero else torch.randn_like(p) * 0.3)
        if not zero:
            st = opt.state[p]
            if kind == 'adamw':
                st['exp_avg'].copy_(torch.randn_like(p) * 0.1)
                st['exp_avg_sq'].copy_(torch.rand_like(p) * 0.01)
            else:
                st['momentum_buffer'].copy_(torch.randn_like(p))
    if kind == 'adamw':
        opt._step_t.fill_(7.0)
    before = [(p.detach().double(), g.double()) + tuple(opt.state[p][k].double()
                                                        for k in opt.STATE)
              for p, g in zip(params, grads)]
    p0_unused = unused.detach().clone()
    opt.step(grads=grads)
    assert opt._table is not None and opt._deferred is None
    worst = {}

    def within(name, got, want, k, s):
        err = (got.double() - want).abs()
        ratio = float((err / (U * s)).nan_to_num(0.0).max()) if err.numel() else 0.0
        worst[name] = max(worst.get(name, 0.0), ratio)
        return bool((err <= k * U * s).all())
    ok = True
    for p, row in zip(params, before):
        st = opt.state[p]
        if kind == 'adamw':
            a, g, c, d = row
            t = 8.0
            c64 = c * B1 + (1 - B1) * g
            s_c = c.abs() * B1 + (1 - B1) * g.abs()
            d64 = d * B2 + (1 - B2) * g * g
            den = d64.sqrt() + EPS
            ss = lr * math.sqrt(1 - B2 ** t) / (1 - B1 ** t)
            a1 = a - ss * (c64 / den)
            a64 = a1 - a1 * (lr * WD)
            s_a = a.abs() + ss * s_c / den + a1.abs() * (lr * WD)
            ok &= within('exp_avg', st['exp_avg'], c64, 5, s_c)
            ok &= within('exp_avg_sq', st['exp_avg_sq'], d64, 6, d64)
            ok &= within('param', p.detach(), a64, 21, s_a)
        else:
            a, g, c = row
            c64 = c * MOM + g + WD * a
            s_c = c.abs() * MOM + g.abs() + WD * a.abs()
            a64 = a - lr * c64
            s_a = a.abs() + lr * s_c
            ok &= within('momentum_buffer', st['momentum_buffer'], c64, 6, s_c)
            ok &= within('param', p.detach(), a64, 9, s_a)
    print(kind, 'worst |err| / (u S):', worst)
    assert ok, worst
    st = opt.state[unused]
    if kind == 'adamw':
        assert float(opt._step_t) == 8.0
        decay = torch.tensor(lr * WD, dtype=torch.float64, device=gpu).float()
        assert torch.equal(unused.detach(), p0_unused - p0_unused * decay)
        assert not st['exp_avg'].any() and not st['exp_avg_sq'].any()
    else:
        f32 = lambda v: torch.tensor(v, dtype=torch.float64, device=gpu).float()
        buf = p0_unused * f32(WD)
        assert torch.equal(st['momentum_buffer'], buf)
        assert torch.equal(unused.detach(), p0_unused - buf * f32(lr))


# ---- 3. graph replay -----------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_graph_replay_equals_eager_steps(gpu, kind):
    """A captured opt.step() replayed twice, with new gradient contents and a
    new lr.fill_ between the replays, equals two eager device steps bit for
    bit (parameters, state, a step count of 3 after the table-building step);
    then a captured step(grads=...) at new addresses, which finish_capture()
    makes the replay read."""
    torch.manual_seed(33)
    src = nn.Sequential(nn.Linear(64, 32), nn.Linear(32, 8)).to(gpu)
    net_e, net_g = copy.deepcopy(src), copy.deepcopy(src)
    pe, pg = list(net_e.parameters()), list(net_g.parameters())
    opt_e, opt_g = _device(kind, pe, gpu), _device(kind, pg, gpu)
    for ps, opt in ((pe, opt_e), (pg, opt_g)):
        _set_grads(ps, [torch.zeros_like(p) for p in ps])
        opt.step()                    # lr 0, zero grads: builds the table
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.step()
    for lr in (1e-3, 5e-4):
        grads = [torch.randn_like(p) for p in pe]
        for ps, opt in ((pe, opt_e), (pg, opt_g)):
            opt.param_groups[0]['lr'].fill_(lr)
            _set_grads(ps, grads)
        opt_e.step()
        graph.replay()
    torch.cuda.synchronize()
    _assert_same_state(opt_e, pe, opt_g, pg)
    assert not torch.equal(pe[0], next(src.parameters()))
    if kind == 'adamw':
        assert float(opt_g._step_t) == 3.0 and float(opt_e._step_t) == 3.0
    # step(grads=...) at addresses the table has not seen
    static = [torch.zeros_like(p) for p in pg]
    key = opt_g._table.key
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        opt_g.step(grads=static)
    assert opt_g._deferred is not None and opt_g._table.key == key
    opt_g.finish_capture()
    assert opt_g._deferred is None and opt_g._table.key != key
    grads = [torch.randn_like(p) for p in pe]
    for s, g in zip(static, grads):
        s.copy_(g)
    for opt in (opt_e, opt_g):
        opt.param_groups[0]['lr'].fill_(2e-4)
    opt_e.step(grads=grads)
    graph2.replay()
    torch.cuda.synchronize()
    _assert_same_state(opt_e, pe, opt_g, pg)
    if kind == 'adamw':
        assert float(opt_g._step_t) == 4.0
    assert int(opt_g._counter) == 0


# ---- 4. load_state_dict --------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_load_state_dict_from_and_into_the_host_class(gpu, kind, tmp_path):
    """A host AdamW / SGD state (two CPU steps; the last parameter never had a
    gradient, so it has no state: zeros here) through torch.save and
    torch.load(map_location='cpu', weights_only=True): the lr stays the
    group's float64 device tensor holding the saved value, and a HIP graph
    captured BEFORE the load continues the saved optimiser bit for bit against
    an eager device optimiser that loaded the same file.  Back: the device
    class's state_dict() loads into the host class, and one further host step
    matches the device step."""
    torch.manual_seed(34)
    src = nn.Sequential(nn.Linear(64, 32), nn.Linear(32, 8))
    host = _host(kind, src.parameters())
    for lr in (1e-3, 5e-4):
        host.param_groups[0]['lr'] = lr
        for p in list(src.parameters())[:-1]:
            p.grad = torch.randn_like(p)
        host.step()
    path = tmp_path / (kind + '.pt')
    torch.save(host.state_dict(), path)
    load = lambda: torch.load(path, map_location='cpu', weights_only=True)
    net_e, net_g = copy.deepcopy(src).to(gpu), copy.deepcopy(src).to(gpu)
    pe, pg = list(net_e.parameters()), list(net_g.parameters())
    # the graph, captured before the load
    opt_g = _device(kind, pg, gpu)
    lr_g = opt_g.param_groups[0]['lr']
    _set_grads(pg, [torch.zeros_like(p) for p in pg])
    opt_g.step()                      # lr 0, zero grads: builds the table
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.step()
    held = [opt_g.state[p][k] for p in pg for k in opt_g.STATE]
    opt_g.load_state_dict(load())
    assert opt_g.param_groups[0]['lr'] is lr_g and lr_g.device.type == 'cuda'
    assert lr_g.dtype == torch.float64 and float(lr_g) == 5e-4
    assert all(a is b for a, b in zip(held, [opt_g.state[p][k] for p in pg
                                             for k in opt_g.STATE]))
    for k in opt_g.STATE:
        assert not opt_g.state[pg[-1]][k].any()
        torch.testing.assert_close(opt_g.state[pg[0]][k].cpu(),
                                   host.state[next(src.parameters())][k], rtol=0, atol=0)
    # eager
    opt_e = _device(kind, pe, gpu)
    opt_e.load_state_dict(load())
    grads = [torch.randn_like(p) for p in pe]
    for ps, opt in ((pe, opt_e), (pg, opt_g)):
        opt.param_groups[0]['lr'].fill_(2e-4)
        _set_grads(ps, grads)
    opt_e.step()
    assert opt_e._table is not None
    graph.replay()
    torch.cuda.synchronize()
    _assert_same_state(opt_e, pe, opt_g, pg)
    assert not torch.equal(pg[0].cpu(), next(src.parameters()))
    if kind == 'adamw':
        assert float(opt_g._step_t) == 3.0 and float(opt_e._step_t) == 3.0
    # back into the host class (on GPU clones), one more step each
    net_h = copy.deepcopy(net_g)
    ph = list(net_h.parameters())
    host2 = _host(kind, ph)
    # (a copy, as a saved file is: Optimizer.load_state_dict keeps tensors
    # that are already on the parameter's device, the device state's own here)
    host2.load_state_dict(copy.deepcopy(opt_g.state_dict()))
    assert host2.param_groups[0]['lr'] == 2e-4
    if kind == 'adamw':
        assert all(host2.state[p]['step'] == 3 for p in ph)
    grads = [torch.randn_like(p) for p in pg]
    opt_g.param_groups[0]['lr'].fill_(1e-4)
    host2.param_groups[0]['lr'] = 1e-4
    _set_grads(pg, grads)
    _set_grads(ph, grads)
    opt_g.step()
    host2.step()
    _assert_close_state(kind, opt_g, pg, host2, ph)


# ---- 5. guards -----------------------------------------------------------------------------
def _stages(g):
    return [s for s, _ in g.read()['stages']]


@pytest.mark.parametrize('kind', KINDS)
def test_step_reports_grad_and_param(gpu, kind):
    """One NaN in a gradient sets the gradient's bit; a finite gradient with an
    lr that overflows the parameters sets the parameters' bit alone."""
    from aido1_amd.guard import Guard
    torch.manual_seed(35)
    g = Guard(gpu)
    p = nn.Parameter(torch.randn(5000, device=gpu))
    opt = _device(kind, [p], gpu)
    opt.set_guard(g, 'critic_grad', 'critic_param')
    opt.param_groups[0]['lr'].fill_(1e-3)
    p.grad = torch.randn_like(p)
    opt.step()
    assert _stages(g) == []
    p.grad[4097] = NAN
    opt.step()
    assert 'critic_grad' in _stages(g)

    g = Guard(gpu)
    p = nn.Parameter(torch.randn(5000, device=gpu))
    opt = _device(kind, [p], gpu)
    opt.set_guard(g, 'actor_grad', 'actor_param')
    opt.param_groups[0]['lr'].fill_(1e39)       # float32(lr) is Inf
    p.grad = torch.randn_like(p)
    opt.step()
    assert _stages(g) == ['actor_param']
    assert not bool(torch.isfinite(p).all())
    assert all(bool(torch.isfinite(opt.state[p][k]).all()) for k in opt.STATE)


# ---- 6. the trainer and the training loop --------------------------------------------------
def _trainer(kind, device, **kw):
    """test_trainer.make_trainer with training.optimizer = kind (make_trainer
    reads the golden config itself, so the same construction here)."""
    from aido1_amd.actor import ConfigActor, ConfigCritic
    from aido1_amd.trainer import DDPGTrainer
    cfg = golden('reference_config.json')
    cfg['training']['optimizer'] = kind
    actor = ConfigActor(no_dropout(cfg['model']['actor']))
    critic = ConfigCritic(no_dropout(cfg['model']['critic']))
    actor.load_state_dict(formula_state_dict(actor.state_dict()))
    critic.load_state_dict(formula_state_dict(critic.state_dict()))
    return DDPGTrainer(cfg, actor, critic, device=device, **kw)


NETS = ('actor', 'critic', 'target_actor', 'target_critic')


@pytest.mark.parametrize('kind', ['adam'] + KINDS)
def test_trainer_graph_equals_eager_stages(gpu, kind):
    """graph=True with warmup=1 (updates 2-3 replay the captured HIP graph)
    against warmup=99 (the same stages run eagerly, the same device optimiser
    reading the autograd outputs): losses, TD errors and every state_dict
    entry over three updates.  The yardstick is "adam" before dt_adamw / dt_sgd
    existed: bit for bit (measured on an MI355X: the largest deviation of any
    loss, TD error or state_dict entry is 0), so all three kinds are held to
    torch.equal."""
    from aido1_amd.optim import DeviceStep
    torch.backends.cudnn.allow_tf32 = False
    cap = _trainer(kind, gpu, graph=True, warmup=1)
    eag = _trainer(kind, gpu, graph=True, warmup=99)
    assert isinstance(cap.actor_optim, DeviceStep) and isinstance(cap.critic_optim, DeviceStep)
    batch = formula_batch(16)
    dev = {}
    same = True

    def cmp(name, a, b):
        nonlocal same
        d = float((a.double() - b.double()).abs().max()) if a.numel() else 0.0
        dev[name] = max(dev.get(name, 0.0), d)
        same = same and torch.equal(a, b)
    for _ in range(3):
        m1, i1 = cap.update(batch)
        m2, i2 = eag.update(batch)
        torch.cuda.synchronize()
        for k in ('critic_loss', 'actor_loss'):
            cmp(k, m1[k], m2[k])
        cmp('td_error', i1['td_error'], i2['td_error'])
    for name in NETS:
        sa, sb = getattr(cap, name).state_dict(), getattr(eag, name).state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            cmp(name, sa[k], sb[k])
    print(kind, 'largest deviation, graph against eager stages:', dev)
    assert cap._graphs is not None and len(cap._graphs) == 1 and eag._graphs is None
    assert same, dev


@pytest.mark.parametrize('kind', KINDS)
def test_trainer_first_update_against_the_host_optimiser(gpu, kind):
    """After update 1 only (later float32 updates are chaotic,
    tests/test_trainer.py), the parameters of the GPU graph-mode trainer (the
    device optimiser) against a CPU graph=False trainer of the same kind (the
    host optimiser), in check_against_reference's float32 scheme: every
    compared summary entry within 2 lr + atol + rtol max|ref| (lr <= 0.004,
    atol = rtol = 1e-3), and at least 90 % of them within atol + rtol |ref|.
    Two CPU trainers agree exactly (tests/test_optim_device.py), so the 90 %
    is a floor the GPU side has to meet."""
    torch.backends.cudnn.allow_tf32 = False
    rtol = atol = 1e-3
    batch = formula_batch(16)
    tr = _trainer(kind, gpu, graph=True, warmup=1)
    ref = _trainer(kind, 'cpu', graph=False)
    tr.update(batch)
    ref.update(batch)
    tr.check()
    bound = 2 * 0.004 + atol
    close, total, worst = 0, 0, 0.0
    for name in NETS:
        got, want = param_summary(getattr(tr, name)), param_summary(getattr(ref, name))
        assert list(got) == list(want), name
        for key, vals in want.items():
            skip = 2 if key.endswith(('kernel.bias', 'running_mean')) else 1
            g, r = np.asarray(got[key])[skip:], np.asarray(vals)[skip:]
            d = np.abs(g - r)
            worst = max(worst, float(d.max()))
            assert d.max() <= bound + rtol * np.abs(r).max(), (name + key, d.max())
            close += int(np.sum(d <= atol + rtol * np.abs(r)))
            total += d.size
    print(kind, 'largest difference %.3g, %d of %d entries close' % (worst, close, total))
    assert close >= 0.9 * total, (close, total)
    init = _trainer(kind, 'cpu', graph=False)
    w = lambda t: t.actor.net.input_nets[0].internal_modules[0].kernel.weight.detach().cpu()
    assert not torch.equal(w(tr), w(init))


def test_train_loop_runs_with_adamw(gpu):
    """The reference's second configuration's optimiser through TrainLoop with
    its default graph=True: 12 steps, clean guards, moved weights, captured
    graphs."""
    from aido1_amd.optim import DeviceAdamW
    from aido1_amd.train_loop import TrainLoop
    cfg = golden('reference_config.json')
    cfg['training']['optimizer'] = 'adamw'
    loop = TrainLoop(cfg, n_envs=128, device=0, seed=5, buffer_size=1000, batch_size=32)
    assert isinstance(loop.trainer.actor_optim, DeviceAdamW)
    assert isinstance(loop.trainer.critic_optim, DeviceAdamW)
    conv = lambda: loop.trainer.actor.net.input_nets[0].internal_modules[0].kernel.weight
    w0 = conv().detach().clone()
    loop.reset()
    for _ in range(12):
        loop.step()
    rec = loop.check()
    assert rec['tick'] == 12 and loop.updates == 12
    assert torch.isfinite(loop.metrics['critic_loss']) and torch.isfinite(loop.metrics['actor_loss'])
    assert not torch.equal(w0, conv())
    assert loop.trainer._graphs is not None
    assert float(loop.trainer.actor_optim._step_t) == 12.0
