"""The small fully connected tails (include/dthead.h: dt_mlp_fwd,
dt_mlp_fwd_td, dt_mlp_bwd) through the C ABI at the shapes that reach every
forward instantiation and sit on every limit of the host check, against a
float64 restatement written here (`mlp_ref`), with per-element bounds derived
from the kernels' operation order (u = 2^-24; nothing here is measured):

* a forward pre-activation is 16 strided fma chains of ceil(K / 16) terms, four
  butterfly adds and the bias add:
      e_pre = (ceil(K / 16) + 6) u (sum_k |x_k w_k| + |b|);
* through an activation (Lipschitz constant at most 1): e_out = e_pre + r u |out|,
  r = 0 for none, 1 for leaky (one product), 8 for tanhf and for
  1 / (1 + expf(-v));
* the second layer: the same form over n1, on |h| + e_h, plus e_h carried
  through |w2|;
* the backward reads the derivative off the saved output: its error e_d is
  the derivative's own Lipschitz constant times e_out (tanh: 2 |o| e + e^2,
  sigmoid: |1 - 2 o| e + e^2) plus 2 u for its two roundings; for leaky it is
  |1 - slope| where |out| <= e_out (the output's sign may differ) and zero
  elsewhere;
* g2 = dy d2 and g1 = (sum_j g2 w2) d1 carry e_d, the product's rounding and,
  for g1, an fma chain of n2 terms;
* every backward sum (dw1, dx, dw2: fma chains; db: plain adds) of t terms:
      e = (t + 2) u sum |products| + the operands' errors carried through,
  the absolute sums taken on |operand| + its error.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SLOPE = float(np.float32(0.01))
NONE, LEAKY, TANH, SIGMOID = 0, 1, 2, 3
SENTINEL = 12345.0
GAP = 64
DT_E_ARG = -1

# (m, k0, k1, n1, n2, act1, act2, b1, b2)
SHAPES = [
    (16, 300, 0, 300, 8, LEAKY, NONE, True, True),        # <32, 32, 1024>
    (8, 1000, 24, 512, 8, TANH, SIGMOID, True, False),    # <64, 32, 512>, kw2 = 32; K, n1, n2 n1 limits
    (256, 1024, 0, 32, 8, SIGMOID, TANH, False, True),    # m, m n1, m n2 limits
    (8, 1, 0, 1024, 0, TANH, NONE, True, False),          # n1 = 1024 with one layer, K = 1
    (1, 1, 0, 1, 0, NONE, NONE, False, False),            # the smallest
    (2, 8, 1016, 64, 64, NONE, LEAKY, False, True),       # n2 = 64; the k0 / k1 seam in a column block
    (64, 255, 2, 128, 1, LEAKY, TANH, True, True),        # kw1 = 17; the seam off a multiple of 16
]
IDS = ['%dx%d+%d-%d-%d' % s[:5] for s in SHAPES]


# ---- the float64 restatement and its bounds -------------------------------------------------
def _act(code, v):
    if code == LEAKY:
        return torch.where(v > 0, v, v * SLOPE)
    if code == TANH:
        return torch.tanh(v)
    if code == SIGMOID:
        return torch.sigmoid(v)
    return v


def _act_rounding(code, out):
    return {NONE: 0.0, LEAKY: 1.0, TANH: 8.0, SIGMOID: 8.0}[code] * U * out.abs()


def _deriv(code, v, out):
    """(the derivative, from the pre-activation's sign for leaky) in float64."""
    if code == LEAKY:
        return torch.where(v > 0, torch.ones_like(v), torch.full_like(v, SLOPE))
    if code == TANH:
        return 1.0 - out * out
    if code == SIGMOID:
        return out * (1.0 - out)
    return torch.ones_like(v)


def _deriv_err(code, out, e):
    if code == LEAKY:
        return torch.where(out.abs() <= e, torch.full_like(out, abs(1.0 - SLOPE)),
                           torch.zeros_like(out))
    if code == TANH:
        return 2.0 * out.abs() * e + e * e + 2.0 * U
    if code == SIGMOID:
        return (1.0 - 2.0 * out).abs() * e + e * e + 2.0 * U
    return torch.zeros_like(out)


def make_inputs(m, k0, k1, n1, n2, b1, b2, seed):
    gen = torch.Generator().manual_seed(seed)
    r = (lambda *s: torch.randn(*s, generator=gen))
    K = k0 + k1
    return dict(x0=r(m, k0), x1=r(m, k1) if k1 else None, w1=r(n1, K) / math.sqrt(K),
                b1=r(n1) * 0.1 if b1 else None, w2=r(n2, n1) / math.sqrt(n1) if n2 else None,
                b2=r(n2) * 0.1 if (n2 and b2) else None, dy=r(m, n2 or n1))


def mlp_ref(inp, act1, act2):
    """float32 CPU inputs -> {name: (float64 value, per-element bound)}."""
    d = (lambda t: t.double() if t is not None else None)
    x0, x1, w1, b1, w2, b2, dy = (d(inp[k]) for k in ('x0', 'x1', 'w1', 'b1', 'w2', 'b2', 'dy'))
    x = torch.cat([x0, x1], 1) if x1 is not None else x0
    m, K = x.shape
    n1 = w1.shape[0]
    n2 = w2.shape[0] if w2 is not None else 0
    zb1 = b1 if b1 is not None else torch.zeros(n1, dtype=torch.float64)
    v1 = x @ w1.T + zb1
    e_v1 = (math.ceil(K / 16) + 6) * U * (x.abs() @ w1.abs().T + zb1.abs())
    h = _act(act1, v1)
    e_h = e_v1 + _act_rounding(act1, h)
    d1 = _deriv(act1, v1, h)
    e_d1 = _deriv_err(act1, h, e_h)
    out = {'h': (h, e_h)}
    if n2:
        zb2 = b2 if b2 is not None else torch.zeros(n2, dtype=torch.float64)
        v2 = h @ w2.T + zb2
        e_v2 = (math.ceil(n1 / 16) + 6) * U * ((h.abs() + e_h) @ w2.abs().T + zb2.abs()) \
            + e_h @ w2.abs().T
        y = _act(act2, v2)
        e_y = e_v2 + _act_rounding(act2, y)
        out['y'] = (y, e_y)
        d2 = _deriv(act2, v2, y)
        e_d2 = _deriv_err(act2, y, e_y)
        g2 = dy * d2
        e_g2 = dy.abs() * e_d2 + U * (g2.abs() + dy.abs() * e_d2)
        a2 = g2.abs() + e_g2
        s = g2 @ w2
        e_s = (n2 + 2) * U * (a2 @ w2.abs()) + e_g2 @ w2.abs()
        g1 = s * d1
        e_g1 = e_s * d1.abs() + (s.abs() + e_s) * e_d1
        e_g1 = e_g1 + U * (g1.abs() + e_g1)
        ah = h.abs() + e_h
        out['dw2'] = (g2.T @ h, (m + 2) * U * (a2.T @ ah) + e_g2.T @ ah + g2.abs().T @ e_h)
        out['db2'] = (g2.sum(0), (m + 2) * U * a2.sum(0) + e_g2.sum(0))
    else:
        g1 = dy * d1
        e_g1 = dy.abs() * e_d1 + U * (g1.abs() + dy.abs() * e_d1)
    a1 = g1.abs() + e_g1
    out['dw1'] = (g1.T @ x, (m + 2) * U * (a1.T @ x.abs()) + e_g1.T @ x.abs())
    out['db1'] = (g1.sum(0), (m + 2) * U * a1.sum(0) + e_g1.sum(0))
    out['dx'] = (g1 @ w1, (n1 + 2) * U * (a1 @ w1.abs()) + e_g1 @ w1.abs())
    return out


@functools.lru_cache(maxsize=None)
def _case(i):
    m, k0, k1, n1, n2, act1, act2, b1, b2 = SHAPES[i]
    inp = make_inputs(m, k0, k1, n1, n2, b1, b2, seed=100 + i)
    return inp, mlp_ref(inp, act1, act2)


# ---- the calls ------------------------------------------------------------------------------
def _lib():
    from aido1_amd import _lib as lib_mod
    return lib_mod


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _struct(shape, dev_inp, slope=SLOPE):
    m, k0, k1, n1, n2, act1, act2 = shape[:7]
    return _lib().DtMlp(m, k0, k1, n1, n2, act1, act2, slope, _ptr(dev_inp['w1']),
                        _ptr(dev_inp['b1']), _ptr(dev_inp['w2']), _ptr(dev_inp['b2']))


class Arena:
    """Output buffers carved out of one sentinel-filled tensor, GAP sentinels
    before, between and after them."""

    def __init__(self, dev, sizes):
        self.off, at = {}, GAP
        for name, n in sizes.items():
            self.off[name] = (at, n)
            at += n + GAP
        self.buf = torch.full((at,), SENTINEL, device=dev)

    def get(self, name):
        at, n = self.off[name]
        return self.buf[at:at + n]

    def untouched_outside(self, written):
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        for name in written:
            at, n = self.off[name]
            keep[at:at + n] = False
        return bool((self.buf[keep] == SENTINEL).all())


def _forward(dev, shape, di, td=None):
    m, k0, k1, n1, n2 = shape[:5]
    sizes = {'h': m * n1, 'y': m * n2, 'target': m * (n2 or n1)}
    ar = Arena(dev, sizes)
    p = _struct(shape, di)
    L = _lib().lib()
    y = ar.get('y') if n2 else None
    if td is None:
        rc = L.dt_mlp_fwd(ctypes.byref(p), _ptr(di['x0']), _ptr(di['x1']), _ptr(ar.get('h')),
                          _ptr(y), _stream(dev))
    else:
        rew, notdone, gamma = td
        rc = L.dt_mlp_fwd_td(ctypes.byref(p), _ptr(di['x0']), _ptr(di['x1']), _ptr(ar.get('h')),
                             _ptr(y), _ptr(rew), _ptr(notdone), gamma, _ptr(ar.get('target')),
                             _stream(dev))
    assert rc == 0
    written = ['h'] + (['y'] if n2 else []) + (['target'] if td is not None else [])
    assert ar.untouched_outside(written)
    return ar.get('h').view(m, n1), (y.view(m, n2) if n2 else None), ar.get('target')


BWD_OUT = ('dx0', 'dx1', 'dw1', 'db1', 'dw2', 'db2')


def _backward(dev, shape, di, h, y, dy, want=BWD_OUT):
    m, k0, k1, n1, n2 = shape[:5]
    sizes = {'dx0': m * k0, 'dx1': m * k1, 'dw1': n1 * (k0 + k1), 'db1': n1, 'dw2': n2 * n1,
             'db2': n2}
    want = [w for w in want if sizes[w] > 0]
    ar = Arena(dev, sizes)
    p = _struct(shape, di)
    ptrs = [_ptr(ar.get(w)) if w in want else None for w in BWD_OUT]
    rc = _lib().lib().dt_mlp_bwd(ctypes.byref(p), _ptr(di['x0']), _ptr(di['x1']), _ptr(h), _ptr(y),
                                 _ptr(dy), *ptrs, _stream(dev))
    assert rc == 0
    assert ar.untouched_outside(want), want
    return {w: ar.get(w).clone() for w in want}


def _to(dev, inp):
    return {k: (v.to(dev) if v is not None else None) for k, v in inp.items()}


def _within(name, got, ref):
    want, bound = ref
    err = (got.double().cpu().reshape(want.shape) - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print('%s: worst error %.3g of its bound' % (name, worst))
    assert bool((err <= bound).all()), '%s: worst error %.3g of its bound' % (name, worst)


@pytest.mark.parametrize('i', range(len(SHAPES)), ids=IDS)
def test_forward_and_backward_within_derived_bounds(gpu, i):
    shape = SHAPES[i]
    m, k0, k1, n1, n2 = shape[:5]
    inp, ref = _case(i)
    di = _to(gpu, inp)
    h, y, _ = _forward(gpu, shape, di)
    _within('h', h, ref['h'])
    if n2:
        _within('y', y, ref['y'])
    g = _backward(gpu, shape, di, h, y, di['dy'])
    dx = torch.cat([g['dx0'].view(m, k0)] + ([g['dx1'].view(m, k1)] if k1 else []), 1)
    _within('dx', dx, ref['dx'])
    for name in ('dw1', 'db1') + (('dw2', 'db2') if n2 else ()):
        _within(name, g[name], ref[name])


@pytest.mark.parametrize('i', range(len(SHAPES)), ids=IDS)
def test_backward_is_homogeneous_and_any_output_may_be_null(gpu, i):
    """dy * 2^-30 gives every gradient times 2^-30 bit for bit; any subset of
    the outputs alone is bit-identical to the all-outputs call, and the
    sentinels around the buffers (`_backward`) stay."""
    shape = SHAPES[i]
    inp, _ = _case(i)
    di = _to(gpu, inp)
    h, y, _ = _forward(gpu, shape, di)
    full = _backward(gpu, shape, di, h, y, di['dy'])
    k = 2.0 ** -30
    small = _backward(gpu, shape, di, h, y, di['dy'] * k)
    for name, v in full.items():
        assert torch.isfinite(v).all()
        assert torch.equal((v * k).view(torch.int32), small[name].view(torch.int32)), name
    for want in (('dx0',), ('dx1',), ('dw1',), ('db1', 'db2'), ('dw2',), ('dx0', 'db1'), ()):
        part = _backward(gpu, shape, di, h, y, di['dy'], want)
        for name, v in part.items():
            assert torch.equal(v.view(torch.int32), full[name].view(torch.int32)), (want, name)


@pytest.mark.parametrize('i', range(len(SHAPES)), ids=IDS)
def test_td_target_from_the_kernels_own_output(gpu, i):
    """dt_mlp_fwd_td: h and y are dt_mlp_fwd's bit for bit, and target is
    float32 rew + (notdone * gamma) * y formed from them, notdone 0 and 1."""
    shape = SHAPES[i]
    m, n1, n2 = shape[0], shape[3], shape[4]
    inp, _ = _case(i)
    di = _to(gpu, inp)
    h0, y0, _ = _forward(gpu, shape, di)
    gen = torch.Generator().manual_seed(i)
    rew = torch.randn(m, generator=gen)
    notdone = (torch.arange(m) % 3 != 1).float()
    gamma = 0.99
    h, y, target = _forward(gpu, shape, di, td=(rew.to(gpu), notdone.to(gpu), gamma))
    assert torch.equal(h.view(torch.int32), h0.view(torch.int32))
    out = h
    if n2:
        assert torch.equal(y.view(torch.int32), y0.view(torch.int32))
        out = y
    out = out.cpu()
    want = rew[:, None] + (notdone * torch.tensor(gamma, dtype=torch.float32))[:, None] * out
    assert torch.equal(target.cpu().view(out.shape).view(torch.int32), want.view(torch.int32))


def _refusal_cases():
    ok = dict(m=1, k0=8, k1=0, n1=8, n2=1, act1=LEAKY, act2=NONE, slope=SLOPE, w2=True)
    cases = {
        'm=257': dict(m=257, n2=0),
        'K=1025': dict(k0=1025),
        'K=1000+25': dict(k0=1000, k1=25),
        'n1=1025': dict(n1=1025, n2=0),
        'n1=513 two layers': dict(n1=513),
        'n2=65': dict(n1=16, n2=65),
        # 8193 = 3 * 2731 and 2049 = 3 * 683 have no factorisation inside the
        # other limits: the least products over the limit that have one
        'm*n1=8194': dict(m=17, n1=482, n2=0),
        'm*n2=2050': dict(m=50, n2=41),
        'n2*n1=4097': dict(n1=241, n2=17),
        'slope<0': dict(slope=-0.01),
        'act1=4': dict(act1=4),
        'act2=4': dict(act2=4),
        'act1=-1': dict(act1=-1),
        'w2 NULL': dict(w2=False),
    }
    return [(k, dict(ok, **v)) for k, v in cases.items()]


def test_over_limit_shapes_are_refused(gpu):
    """Each limit of the host check plus one, a negative slope, an unknown
    activation and a missing w2: DT_E_ARG from all three entry points (no
    kernel runs; all-zero buffers of legal size), the shape they leave legal
    accepted."""
    L = _lib().lib()
    zero = torch.zeros(1 << 21, device=gpu)
    z = zero.data_ptr()

    def call(c):
        p = _lib().DtMlp(c['m'], c['k0'], c['k1'], c['n1'], c['n2'], c['act1'], c['act2'],
                         c['slope'], z, z, z if c['w2'] else None, z)
        s = _stream(gpu)
        x1 = z if c['k1'] else None
        return (L.dt_mlp_fwd(ctypes.byref(p), z, x1, z, z, s),
                L.dt_mlp_fwd_td(ctypes.byref(p), z, x1, z, z, z, z, 0.99, z, s),
                L.dt_mlp_bwd(ctypes.byref(p), z, x1, z, z, z, z, x1, z, z, z, z, s))
    for name, c in _refusal_cases():
        assert call(c) == (DT_E_ARG,) * 3, name
    torch.cuda.synchronize()
    assert not zero.any()
    ok = dict(m=1, k0=8, k1=0, n1=8, n2=1, act1=LEAKY, act2=NONE, slope=SLOPE, w2=True)
    assert call(ok) == (0, 0, 0)
    torch.cuda.synchronize()
