"""The fp16 actor convolutions (aido1_amd/csrc/dtconv.hip: dt_conv1_split,
dt_conv32_split) bit for bit on exact-arithmetic inputs, layer by layer, in
reference mode (the previous layer's per-sample BatchNorm at the ring commit,
centred outputs, per-sample statistics, conv4's own BatchNorm) and in eval
mode.  tests/actor_exact_ref.py builds the pools and says why a float64
reference rounded once to fp16 must equal the kernel's output;
tests/test_actor_exact_ref.py asserts the conditions.

Every stored output and every centre is compared with torch.equal.  What is
not exact has a tolerance of four times a CPU float32 restatement's error
against float64 (actor_exact_ref.K_STAT, K_OUT4, measured there):

  statistics of conv1..conv3   |mean err| <= K u max|d|,  |M2 err| <= K u M2
  conv4's normalised output    |err| <= 2^-11 |want| + K u (|v| sc + mean|v| sc + |out_beta|)

The kernels' own worst error over those bounds on an MI355X (printed by the
tests before they assert) is under RATIOS below.

Sample i of a launch is pool[a[i]] with a seeded random a, so neighbouring
samples differ and the expectation is a gather.  Sample counts, with CU the
device's compute units: n in {1, 2, 3, 19, 5 CU // 2 + 3, 9 CU + 5}.  The
persistent grid is per x CU workgroups (per = the kernel's occupancy) and
workgroup b takes samples b, b + grid, ...; samples per workgroup (min-max):

  per   n = 5 CU // 2 + 3      n = 9 CU + 5
  1     2-3                    9-10
  2     1-2                    4-5
  3     0-1                    3-4
  4     0-1                    2-3

so at the occupancies the kernels have (conv1 and conv4 two, conv2 / conv3 two
or three) some workgroup reaches its fourth sample (the k % 3 statistics
buffer wraps, conv1's 120-row samples pass through all four phases of the
32-row ring, conv2..4's ring phase (k IH + r) % kRing cycles), and conv4 runs
both an even and an odd total >= 3 through its two-step unrolled loop; n = 2
and n = 3 on one workgroup each are total 1 (no prologue special case), and
the small counts put one sample in each workgroup.

Canaries: y and part carry a tail of TAIL bytes of a sentinel after the last
sample (invalid lanes store at the sample's kBytes, which the buffer range
check must drop) and are filled with the sentinel before the launch; conv1's
ring slots that `order` does not name are NaN.

RATIOS (MI355X, worst observed error / bound over every case): statistics
mean 0.247 / M2 0.248 (conv1), 0.244 / 0.248 (conv2), 0.245 / 0.248 (conv3),
that is the kernels' float32 statistics err exactly as the CPU restatement
does, a quarter of the bound; conv4's normalised output 0.992, where the fp16
store's 2^-11 |want| is the whole of it (a half ulp just above a power of
two); the real-valued cases 0.211 (conv2), 0.205 (conv3), 0.050 (conv4).
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import actor_exact_ref as R

pytestmark = pytest.mark.gpu

TAIL = 4096                     # bytes of sentinel after the last sample
S16, S32 = 0x5A5A, 0x5A5A5A5A   # the sentinel as fp16 / float32 bits
COUNTS = ['1', '2', '3', '19', '5cu/2+3', '9cu+5']
_DEV = {}


@pytest.fixture(scope='module', autouse=True)
def _release_device_memory():
    """The device pools and the launch buffers of the largest counts (a few GB
    in the caching allocator) go back to the driver after the module."""
    yield
    _DEV.clear()
    torch.cuda.empty_cache()


def _count(name, gpu):
    cu = torch.cuda.get_device_properties(gpu).multi_processor_count
    return {'5cu/2+3': 5 * cu // 2 + 3, '9cu+5': 9 * cu + 5}.get(name) or int(name)


def _lib():
    from aido1_amd import _lib as m
    return m.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _pool(gpu, layer, seed=0, eps=0.0):
    """The pool's tensors on the device (float64 references computed once on
    the CPU, moved once a module run) with the layer's weight fragments."""
    from aido1_amd.actor import conv1_fragments, conv32_fragments
    key = (layer, seed, eps)
    if key not in _DEV:
        src = R.pool1(seed) if layer == 1 else R.pool32(layer, seed, eps)
        p = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in src.items()}
        p['wf'] = (conv1_fragments if layer == 1 else conv32_fragments)(p['w']).contiguous()
        _DEV[key] = p
    return _DEV[key]


def _picks(n, seed):
    return torch.from_numpy(np.random.default_rng([n, seed]).integers(0, R.P, n))


def _canary(count, dtype, gpu):
    """`count` elements plus the tail, all sentinel: (whole, the count elements)."""
    if dtype == torch.float16:
        whole = torch.full((count + TAIL // 2,), S16, dtype=torch.int16, device=gpu)
    else:
        whole = torch.full((count + TAIL // 4,), S32, dtype=torch.int32, device=gpu)
    return whole, whole.view(dtype)[:count]


def _tail_untouched(whole, count):
    sentinel = S16 if whole.dtype == torch.int16 else S32
    assert bool((whole[count:] == sentinel).all()), 'the kernel wrote past its last sample'


def _same(got, want, n, what, pixels=None):
    """Equality of two [n, ...] tensors (fp16 by their bits); on failure the
    number of mismatches and the first (sample, pixel, channel)."""
    if got.dtype == torch.float16:
        got, want = got.view(torch.int16), want.view(torch.int16)
    got, want = got.reshape(n, -1), want.reshape(n, -1)
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    s, e = bad[0].tolist()
    px, ch = divmod(e, 32) if pixels is None else (e % pixels, e // pixels)
    pytest.fail('%s: %d of %d values differ, first at sample %d pixel %d channel %d '
                '(got bits/value %r, want %r)' % (what, bad.shape[0], got.numel(), s, px, ch,
                                                  got[s, e].item(), want[s, e].item()))


def _stats_ok(part, pool, a, layer, what):
    """(mean, M2) of the kernel against float64 of the exact centred values."""
    km, kq = R.K_STAT[layer]
    worst = []
    for col, k, ref, unit in ((0, km, pool['mean'][a], pool['dmax'][a]),
                              (1, kq, pool['m2'][a], pool['m2'][a])):
        err = (part[..., col].double() - ref).abs()
        bound = k * R.U * unit
        nz = bound > 0
        worst.append((err[nz] / bound[nz]).max().item() if nz.any() else 0.0)
        assert bool((err <= bound).all()), (what, 'mean M2'.split()[col], worst)
    print('%s: statistics error / bound: mean %.3f M2 %.3f' % (what, *worst))


def _split(n0, p2, layer):
    from aido1_amd import _lib as m
    if layer == 1:
        return ctypes.byref(m.DtConvSet(n0, p2['wf'].data_ptr(), p2['b'].data_ptr()))
    last = layer == 4
    return ctypes.byref(m.DtConvSet(n0, p2['wf'].data_ptr(), p2['b'].data_ptr(),
                                    p2['gamma'].data_ptr(), p2['beta'].data_ptr(),
                                    p2['og'].data_ptr() if last else None,
                                    p2['ob'].data_ptr() if last else None))


def _mix(key, p, a, p2=None, n0=None):
    """pool[key][a] on the device; rows [n0, n) from the second pool."""
    a = a.to(p[key].device)
    if p2 is None:
        return p[key][a]
    return torch.cat([p[key][a[:n0]], p2[key][a[n0:]]])


def _run1(gpu, p, a, slots, order, stats, p2=None, n0=None):
    """dt_conv1_split on ring samples pool[a]; returns (y [n, 57, 77, 32], part)."""
    n = a.shape[0]
    ring = torch.full((n, slots, 120, 160), float('nan'), device=gpu)
    ring[:, order] = _mix('frames', p, a, p2, n0)
    ywhole, y = _canary(n * 57 * 77 * 32, torch.float16, gpu)
    pwhole, part = _canary(n * 96, torch.float32, gpu) if stats else (None, None)
    o = (ctypes.c_int32 * 3)(*order)
    rc = _lib().dt_conv1_split(ring.data_ptr(), n, slots, o, p['wf'].data_ptr(), p['b'].data_ptr(),
                               _split(n0, p2, 1) if p2 else None, y.data_ptr(), _ptr(part),
                               R.SLOPE, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    _tail_untouched(ywhole, y.numel())
    if stats:
        _tail_untouched(pwhole, part.numel())
        part = part.view(n, 32, 3)
    return y.view(n, 57, 77, 32), part


def _run32(gpu, layer, p, a, mode, p2=None, n0=None, prev=None, wf=None):
    """dt_conv32_split on samples pool[a]: mode 'ref' (the previous layer's
    statistics, in_eps = the pool's) or 'eval'.  Returns (y, part)."""
    n = a.shape[0]
    oh, ow = R.GEOM[layer][2:4]
    ref = mode == 'ref'
    x = _mix('x16' if ref else 'xe16', p, a, p2, n0).contiguous()
    if ref and prev is None:
        prev = _mix('prev', p, a, p2, n0).contiguous()
    ywhole, y = _canary(n * oh * ow * 32, torch.float16, gpu)
    stats = ref and layer != 4
    pwhole, part = _canary(n * 96, torch.float32, gpu) if stats else (None, None)
    last = ref and layer == 4
    rc = _lib().dt_conv32_split(
        layer, n, x.data_ptr(), (p['wf'] if wf is None else wf).data_ptr(),
        (p['b'] if ref else p['be']).data_ptr(), _ptr(prev),
        p['gamma'].data_ptr() if ref else None, p['beta'].data_ptr() if ref else None,
        p['eps'] if ref else 0.0, y.data_ptr(), _ptr(part),
        p['og'].data_ptr() if last else None, p['ob'].data_ptr() if last else None,
        R.EPS if last else 0.0, R.SLOPE, _split(n0, p2, layer) if p2 else None, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    _tail_untouched(ywhole, y.numel())
    if stats:
        _tail_untouched(pwhole, part.numel())
        part = part.view(n, 32, 3)
    return (y.view(n, 32 * oh * ow) if layer == 4 else y.view(n, oh, ow, 32)), part


def _out4_bad(y, p, a, p2=None, n0=None):
    """conv4's normalised output against float64: the elements over the bound
    [n, 4032] (bool) and the worst error / bound."""
    want = _mix('want', p, a, p2, n0)
    bound = 2.0 ** -11 * want.abs() + R.K_OUT4 * R.U * _mix('unit', p, a, p2, n0)
    err = (y.double() - want).abs()
    return err > bound, (err / bound).max().item()


def _check32(layer, mode, y, part, p, a, what, p2=None, n0=None):
    n = a.shape[0]
    pixels = R.GEOM[layer][2] * R.GEOM[layer][3]
    if mode == 'eval':
        _same(y, _mix('ye', p, a, p2, n0), n, what + ' y', pixels if layer == 4 else None)
        return
    if layer == 4:
        assert bool(torch.isfinite(y).all()), what
        bad, worst = _out4_bad(y, p, a, p2, n0)
        print('%s: normalised output error / bound %.3f' % (what, worst))
        assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[0].tolist(), worst)
        for q, sl in ((p, slice(0, n0)), (p2, slice(n0, n))) if p2 else ((p, slice(0, n)),):
            for co in R.ZERO_CO:     # a flat channel normalises to exactly out_beta
                got = y.view(n, 32, pixels)[sl, co]
                assert bool((got == q['ob'][co].half()).all()), (what, co)
        return
    _same(y, _mix('y', p, a, p2, n0), n, what + ' y')
    want_part = _mix('part', p, a, p2, n0)
    _same(part[..., 2].contiguous(), want_part[..., 2].float().contiguous(), n, what + ' centre',
          pixels=1)
    for q, sl in ((p, slice(0, n0)), (p2, slice(n0, n))) if p2 else ((p, slice(0, n)),):
        _stats_ok(part[sl], q, a[sl].to(part.device), layer, what)
    for co in R.ZERO_CO:             # zero weights: (0, 0, c) exactly
        assert bool((part[:, co, :2] == 0).all()), (what, co)


@pytest.mark.parametrize('stats', [True, False], ids=['ref', 'eval'])
@pytest.mark.parametrize('slots,order', [(4, [2, 3, 0]), (3, [1, 0, 2])])
@pytest.mark.parametrize('count', COUNTS)
def test_conv1_is_exact(gpu, count, slots, order, stats):
    """conv1 from the ring with and without statistics: stored fp16 bits and
    centres equal, (mean, M2) within four times the float32 restatement."""
    n = _count(count, gpu)
    p, a = _pool(gpu, 1), _picks(n, 1)
    y, part = _run1(gpu, p, a, slots, order, stats)
    what = 'conv1 n=%d' % n
    assert bool(torch.isfinite(y).all()), what
    if not stats:
        _same(y, _mix('ye', p, a), n, what + ' y')
        return
    _same(y, _mix('y', p, a), n, what + ' y')
    _same(part[..., 2].contiguous(), _mix('part', p, a)[..., 2].float().contiguous(), n,
          what + ' centre', pixels=1)
    _stats_ok(part, p, a.to(gpu), 1, what)
    for co in R.ZERO_CO:
        assert bool((part[:, co, :2] == 0).all()), (what, co)


@pytest.mark.parametrize('mode', ['ref', 'ref-eps', 'eval'])
@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('layer', [2, 3, 4])
def test_conv32_is_exact(gpu, layer, count, mode):
    """conv2..conv4 per layer: reference mode (in_eps = 0), its flat-channel
    variant (in_eps = 1e-5: the flat input channel stages exactly beta) and
    eval mode.  Layers 2 / 3 and eval-mode conv4: bits equal; reference-mode
    conv4: its own BatchNorm's output within the derived bound."""
    n = _count(count, gpu)
    p = _pool(gpu, layer, 0, 1e-5 if mode == 'ref-eps' else 0.0)
    a = _picks(n, layer)
    run = 'eval' if mode == 'eval' else 'ref'
    y, part = _run32(gpu, layer, p, a, run)
    _check32(layer, run, y, part, p, a, 'conv%d %s n=%d' % (layer, mode, n))


@pytest.mark.parametrize('case', ['n3-n0=1', 'n3-n0=2', 'big-n0=1', 'big-n0=n-1'])
@pytest.mark.parametrize('layer', [1, 2, 3, 4])
def test_two_weight_sets_are_exact(gpu, layer, case):
    """One launch over two exact weight sets in reference mode: every sample
    gets the expectation of its own set (not merely what a launch of its own
    gives, as test_split_launch_matches_separate_actors checks)."""
    n = 3 if case.startswith('n3') else _count('5cu/2+3', gpu)
    n0 = {'n3-n0=1': 1, 'n3-n0=2': 2, 'big-n0=1': 1, 'big-n0=n-1': n - 1}[case]
    p, p2 = _pool(gpu, layer, 0), _pool(gpu, layer, 1)
    a = _picks(n, 10 + layer)
    what = 'conv%d split n=%d n0=%d' % (layer, n, n0)
    if layer == 1:
        y, part = _run1(gpu, p, a, 3, [2, 0, 1], True, p2, n0)
        _same(y, _mix('y', p, a, p2, n0), n, what + ' y')
        _same(part[..., 2].contiguous(), _mix('part', p, a, p2, n0)[..., 2].float().contiguous(),
              n, what + ' centre', pixels=1)
        _stats_ok(part[:n0], p, a[:n0].to(gpu), 1, what)
        _stats_ok(part[n0:], p2, a[n0:].to(gpu), 1, what)
        return
    y, part = _run32(gpu, layer, p, a, 'ref', p2, n0)
    _check32(layer, 'ref', y, part, p, a, what, p2, n0)


@pytest.mark.parametrize('layer', [2, 3, 4])
def test_one_tap_off_by_a_grain_is_noticed(gpu, layer):
    """Sensitivity (a): the unmodified kernel with one tap of one (co, ci) pair
    moved by TAP_GRAIN before conv32_fragments.  The exact comparison finds
    mismatches, all in channel co; the max-abs tolerance of
    test_conv32_layers_match_conv2d (3e-3 max(1, max |ref|)) does not see the
    change.  Layers 2 / 3 in reference mode, conv4 in eval mode (stored bits)."""
    from aido1_amd.actor import conv32_fragments
    n, co = 19, 9
    p, a = _pool(gpu, layer), _picks(n, 20 + layer)
    w = p['w'].clone()
    w[co, 3, 1, 2] += R.TAP_GRAIN
    mode = 'eval' if layer == 4 else 'ref'
    wf = conv32_fragments(w).contiguous()
    y, part = _run32(gpu, layer, p, a, mode, wf=wf)
    pixels = R.GEOM[layer][2] * R.GEOM[layer][3]
    if layer == 4:
        got, want = y.view(n, 32, pixels), _mix('ye', p, a).view(n, 32, pixels)
        full, ref = got.float(), want.float()
    else:
        got, want = y.view(n, pixels, 32).transpose(1, 2), \
            _mix('y', p, a).view(n, pixels, 32).transpose(1, 2)
        c = part[..., 2]
        full, ref = got.float() + c[..., None], _mix('v', p, a).flatten(2).float()
    diff = got.contiguous().view(torch.int16) != want.contiguous().view(torch.int16)
    assert bool(diff[:, co].any()), 'the exact comparison missed the moved tap'
    diff[:, co] = False
    assert not bool(diff.any()), 'mismatches outside channel %d' % co
    # what the max-abs tolerance makes of the same output
    err = (full - ref).abs().max().item()
    tol = 3e-3 * max(1.0, ref.abs().max().item())
    print('conv%d: moved tap: max |err| %.4f, old tolerance %.4f' % (layer, err, tol))
    assert err < tol


@pytest.mark.parametrize('layer', [2, 3, 4])
def test_swapped_statistics_are_noticed(gpu, layer):
    """Sensitivity (b): two samples' prev_part rows swapped before the launch
    (a sample's statistics taken from its neighbour).  Mismatches in exactly
    those two samples (conv4: elements over its bound)."""
    n = 19
    p, a = _pool(gpu, layer), _picks(n, 30 + layer)
    i = 3
    j = next(k for k in range(i + 1, n) if a[k] != a[i])
    prev = _mix('prev', p, a).clone()
    prev[[i, j]] = prev[[j, i]]
    y, part = _run32(gpu, layer, p, a, 'ref', prev=prev.contiguous())
    if layer == 4:
        bad, _ = _out4_bad(y, p, a)
    else:
        bad = (y.view(torch.int16) != _mix('y', p, a).view(torch.int16)).flatten(1)
    hit = bad.any(1).nonzero().flatten().tolist()
    assert hit == [i, j], hit


@pytest.mark.parametrize('layer', [2, 3, 4])
def test_real_valued_inputs_within_the_elementwise_bound(gpu, layer):
    """Realistic activations (per-channel spreads e^(2 N(0,1)), as the x3
    tests' _layer_case) in reference mode, n = 19, in_eps = 1e-5, against
    float64 of the exactly normalised input xs, elementwise:

      |v_kernel - v| <= (2^-11 + K 2^-24) (|w| * |xs|),  K = 512 + 8

    (2^-11: the staged input's fp16 rounding; 512 float32 accumulations; 8:
    the float32 error of sc and sh), plus 2^-11 |v - c| for the store of the
    centred value.  conv4's own BatchNorm carries that bound e through its
    normalisation: with s = sqrt(var + eps), s' = s - rms(e),

      |err| <= gamma ((e + mean e) / s' + |v - mean| rms(e) / (s s'))
               + 2^-11 |want| + K_OUT4 u (|v| sc + mean|v| sc + |out_beta|)."""
    from aido1_amd.actor import conv32_fragments
    n = 19
    ih, iw, oh, ow, st, _ = R.GEOM[layer]
    g = torch.Generator(device=gpu).manual_seed(100 + layer)
    spread = torch.exp(torch.randn(n, 1, 1, 32, device=gpu, generator=g) * 2.0)
    x16 = (torch.randn(n, ih, iw, 32, device=gpu, generator=g) * spread +
           torch.randn(n, 1, 1, 32, device=gpu, generator=g) * spread).half().contiguous()
    xt = x16.double()
    mean = xt.mean((1, 2))
    m2 = ((xt - mean[:, None, None, :]) ** 2).sum((1, 2))
    prev = torch.stack([mean.float(), m2.float(), torch.zeros_like(mean).float()], -1).contiguous()
    gamma = torch.rand(32, device=gpu, generator=g) + 0.5
    beta = torch.rand(32, device=gpu, generator=g) - 0.5
    w16 = (torch.randn(32, 32, 4, 4, device=gpu, generator=g) * 0.05).half()
    b = torch.randn(32, device=gpu, generator=g) * 0.1
    og = torch.rand(32, device=gpu, generator=g) + 0.5
    ob = torch.rand(32, device=gpu, generator=g) - 0.5
    slope = 0.01
    pm, pv = prev[..., 0].double(), prev[..., 1].double() / (ih * iw)
    xs = ((xt - pm[:, None, None, :]) / torch.sqrt(pv[:, None, None, :] + R.EPS) *
          gamma.double() + beta.double()).permute(0, 3, 1, 2)
    acc = F.conv2d(xs, w16.double(), b.double(), stride=st)
    v = torch.maximum(acc, acc * float(np.float32(slope)))
    e = (2.0 ** -11 + (512 + 8) * R.U) * F.conv2d(xs.abs(), w16.double().abs(), stride=st)

    ywhole, y = _canary(n * oh * ow * 32, torch.float16, gpu)
    last = layer == 4
    pwhole, part = (None, None) if last else _canary(n * 96, torch.float32, gpu)
    wf = conv32_fragments(w16.float()).contiguous()
    rc = _lib().dt_conv32_split(layer, n, x16.data_ptr(), wf.data_ptr(), b.data_ptr(),
                                prev.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-5,
                                y.data_ptr(), _ptr(part), og.data_ptr() if last else None,
                                ob.data_ptr() if last else None, 1e-5 if last else 0.0, slope,
                                None, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    _tail_untouched(ywhole, y.numel())
    assert bool(torch.isfinite(y).all())
    if last:
        vf, ef = v.flatten(2), e.flatten(2)
        mu = vf.mean(-1, keepdim=True)
        s = torch.sqrt(((vf - mu) ** 2).mean(-1, keepdim=True) + R.EPS)
        s_lo = s - torch.sqrt((ef ** 2).mean(-1, keepdim=True))
        assert bool((s_lo > 0.5 * s).all())
        gd, bd = og.double().view(1, 32, 1), ob.double().view(1, 32, 1)
        want = (vf - mu) / s * gd + bd
        unit = (vf.abs() + vf.abs().mean(-1, keepdim=True)) * gd / s + bd.abs()
        bound = gd * ((ef + ef.mean(-1, keepdim=True)) / s_lo +
                      (vf - mu).abs() * (s - s_lo) / (s * s_lo)) + \
            2.0 ** -11 * want.abs() + R.K_OUT4 * R.U * unit
        err = (y.view(n, 32, oh * ow).double() - want).abs()
    else:
        _tail_untouched(pwhole, part.numel())
        part = part.view(n, 32, 3)
        c = part[..., 2].double()
        assert bool(((c - v[:, :, 0, 0]).abs() <= e[:, :, 0, 0]).all())
        got = y.view(n, oh, ow, 32).permute(0, 3, 1, 2).double() + c[:, :, None, None]
        bound = e + 2.0 ** -11 * (v - v[:, :, :1, :1]).abs()
        err = (got - v).abs()
    print('conv%d real-valued: worst error / bound %.3f' % (layer, (err / bound).max().item()))
    assert bool((err <= bound).all()), (int((err > bound).sum()), (err / bound).max().item())
