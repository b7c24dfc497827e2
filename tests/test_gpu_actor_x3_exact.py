"""The float32-accurate "x3" actor kernels (aido1_amd/csrc/dtconvx.hip:
dt_conv1x_split, dt_conv32x_split, dt_actor_head_x3) bit for bit on
exact-arithmetic inputs.  tests/actor_x3_exact_ref.py builds the pools and
says why the float64 three-product model, split as the store splits it, must
equal the kernels' output; tests/test_actor_x3_exact_ref.py asserts the
conditions.  The scheme, the canaries and the helpers are those of the fp16
chain's tests/test_gpu_actor_exact.py.

Every stored (hi, lo) pair (the whole HLB image as int16, the chunks no pixel
owns still holding the sentinel) and every centre is compared for equality,
and so are lin1's partial sums and the head's output.  What is not exact has a
tolerance of four times a CPU float32 restatement's error against float64
(actor_x3_exact_ref.K_STAT, K_OUT4, measured there):

  statistics of conv1..conv3   |mean err| <= K u max|d|,  |M2 err| <= K u M2
  conv4's normalised output    |err| <= K u (|v| sc + mean|v| sc + |out_beta|)

Sample counts, with CU the device's compute units: n in {1, 2, 3, 19,
5 CU // 2 + 3, 6 CU + 5}.  Every x3 convolution kernel is launched on a
persistent grid of per x CU workgroups of 256 threads, per its occupancy
(resident_grid): __launch_bounds__(256, 2) holds conv1x_kernel and the three
conv32x_kernel instantiations (DTCONVX_NW 4, DTCONVX_DEPTH 1) to 256
registers, two workgroups a CU, and their LDS (62 KB: conv1x's hi and lo
rings; 68 KB: conv32x's folded hi and lo fragments) allows no third in 160 KB.
Workgroup b takes samples b, b + grid, ...; samples a workgroup (min-max):

  per   n = 5 CU // 2 + 3      n = 6 CU + 5
  1     2-3                    6-7
  2     1-2                    3-4

so at per = 2 the first large count has workgroups with one and with two
samples (conv1x's prefetch crossing into a next sample or clamping), and the
second, the smallest that does, sends some workgroups to their fourth sample
(the per-sample fold's LDS weights, s_wexp, s_c and the statistics' `red` are
rewritten a fourth time; conv1x's 120-row samples pass all four phases of its
32-row rings) while conv4x runs both an odd and an even total >= 3.  The fp16
file's 9 CU + 5 is that count for its kernels' occupancy of up to three.

Canaries: y, part, the head's work and out carry a tail of TAIL bytes of a
sentinel after the last sample (invalid lanes store at the sample's kBytes,
which the buffer range check must drop) and are filled with the sentinel
before the launch; conv1's ring slots that `order` does not name are NaN.

The fold's branches no other test reaches, at n = 19:
  rescale  max|sc| max|w| > 16384: e = 2 in six pool samples, 0 in one
  subw     folded weights whose hi half is the fp16 subnormal 2^-16
  sublo    inputs whose lo halves are fp16 subnormals (and e up to 3)
  eps      the flat input channel under the fold

Measured by test_rare_fold_branches_are_exact on the MI355X: all three pass, so
v_mfma_f32_32x32x16_f16 keeps fp16-subnormal A and B operands
(tests/test_actor_x3_exact_ref.py shows that flushing them would move most
outputs of those pools); no kernel needed a change.

RATIOS (MI355X, worst observed error / bound over every case): statistics
mean 0.242 / M2 0.248 (conv1x), 0.245 / 0.250 (conv2x), 0.248 / 0.248
(conv3x), conv4x's normalised output 0.249: the kernels' float32 statistics
err as the CPU restatement does, a quarter of the bound.  The real-valued
cases 0.009 (conv1x), 0.004 (conv2x), 0.004 (conv3x), 0.001 (conv4x): the
errors add like a random walk, far under the worst-case K.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import actor_exact_ref as R
import actor_x3_exact_ref as X
from test_gpu_actor_exact import (S16, _canary, _lib, _mix, _picks, _ptr, _stream,
                                  _tail_untouched)

pytestmark = pytest.mark.gpu

COUNTS = ['1', '2', '3', '19', '5cu/2+3', '6cu+5']
HEAD_CASES = [(1, 1), (33, 1), (64, 64), (97, 96), (300, 257)]
_DEV = {}


@pytest.fixture(scope='module', autouse=True)
def _release_device_memory():
    """The device pools and the launch buffers of the largest counts go back
    to the driver after the module."""
    yield
    _DEV.clear()
    torch.cuda.empty_cache()


def _count(name, gpu):
    cu = torch.cuda.get_device_properties(gpu).multi_processor_count
    return {'5cu/2+3': 5 * cu // 2 + 3, '6cu+5': 6 * cu + 5}.get(name) or int(name)


def _out_geom(layer):
    """(OH, OW, the stride the layer's HLB output is read at)."""
    return X.GEOM[layer][2], X.GEOM[layer][3], X.NEXT_STRIDE.get(layer)


def _pool(gpu, layer, seed=0, var='plain'):
    """The pool's tensors on the device (float64 references computed once on
    the CPU, moved once a module run), the layer's weights as the kernel takes
    them and the expected HLB image with the sentinel in its unowned chunks."""
    from aido1_amd.actor import conv1_fragments, conv32_fragments, split_hl
    key = (layer, seed, var)
    if key not in _DEV:
        src = X.pool1x(seed) if layer == 1 else X.pool32x(layer, seed, var)
        names = ('frames', 'xin', 'prev', 'gamma', 'beta', 'w', 'b', 'og', 'ob', 'd32', 'part',
                 'mean', 'm2', 'dmax', 'want', 'unit', 'v', 'layer', 'eps')
        p = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in src.items() if k in names}
        if layer == 1:
            p['wf'] = split_hl(conv1_fragments(p['w'], torch.float32)).contiguous()
        else:
            p['wf'] = conv32_fragments(p['w'], torch.float32).contiguous()
        if layer != 4:
            p['img'] = X.hlb_image(p['d32'], X.NEXT_STRIDE[layer], S16).flatten(1)
        _DEV[key] = p
    return _DEV[key]


def _first_diff(got, want, what):
    """Equality of two [n, ...] tensors of bits; on failure the count and the
    first (sample, flat element)."""
    n = got.shape[0]
    got, want = got.reshape(n, -1), want.reshape(n, -1)
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    s, e = bad[0].tolist()
    pytest.fail('%s: %d of %d values differ, first at sample %d element %d (got %r, want %r)' % (
        what, bad.shape[0], got.numel(), s, e, got[s, e].item(), want[s, e].item()))


def _stats_ok(part, pool, a, layer, what):
    """(mean, M2) of the kernel against float64 of the exact centred values."""
    km, kq = X.K_STAT[layer]
    worst = []
    for col, k, ref, unit in ((0, km, pool['mean'][a], pool['dmax'][a]),
                              (1, kq, pool['m2'][a], pool['m2'][a])):
        err = (part[..., col].double() - ref).abs()
        bound = k * X.U * unit
        nz = bound > 0
        worst.append((err[nz] / bound[nz]).max().item() if nz.any() else 0.0)
    print('%s: statistics error / bound: mean %.3f M2 %.3f' % (what, *worst))
    for col, k, ref, unit in ((0, km, pool['mean'][a], pool['dmax'][a]),
                              (1, kq, pool['m2'][a], pool['m2'][a])):
        err = (part[..., col].double() - ref).abs()
        assert bool((err <= k * X.U * unit).all()), (what, 'mean M2'.split()[col], worst)


def _split(n0, p2, layer):
    from aido1_amd import _lib as m
    if layer == 1:
        return ctypes.byref(m.DtConvSet(n0, p2['wf'].data_ptr(), p2['b'].data_ptr()))
    last = layer == 4
    return ctypes.byref(m.DtConvSet(n0, p2['wf'].data_ptr(), p2['b'].data_ptr(),
                                    p2['gamma'].data_ptr(), p2['beta'].data_ptr(),
                                    p2['og'].data_ptr() if last else None,
                                    p2['ob'].data_ptr() if last else None))


def _hlb_elems(layer):
    from aido1_amd.actor import hlb_shape
    oh, ow, sn = _out_geom(layer)
    return int(np.prod(hlb_shape(1, oh, ow, sn)))


def _launch1x(gpu, ring, index, order, wf, b, set2):
    """dt_conv1x_split on a ring into sentinel-filled y and part; returns (y
    as int16 [n, image], part [n, 32, 3])."""
    n, slots = ring.shape[:2]
    ywhole, y = _canary(n * _hlb_elems(1), torch.float16, gpu)
    pwhole, part = _canary(n * 96, torch.float32, gpu)
    o = (ctypes.c_int32 * 3)(*order)
    rc = _lib().dt_conv1x_split(ring.data_ptr(), int(index), n, slots, o, wf.data_ptr(),
                                b.data_ptr(), set2, y.data_ptr(), part.data_ptr(), X.SLOPE,
                                _stream())
    assert rc == 0
    torch.cuda.synchronize()
    _tail_untouched(ywhole, y.numel())
    _tail_untouched(pwhole, part.numel())
    return y.view(torch.int16).view(n, -1), part.view(n, 32, 3)


def _run1x(gpu, p, a, slots, order, p2=None, n0=None, wf=None):
    n = a.shape[0]
    ring = torch.full((n, slots, 120, 160), float('nan'), device=gpu)
    ring[:, order] = _mix('frames', p, a, p2, n0)
    return _launch1x(gpu, ring, False, order, p['wf'] if wf is None else wf, p['b'],
                     _split(n0, p2, 1) if p2 else None)


def _run32x(gpu, layer, p, a, p2=None, n0=None, prev=None, wf=None, xin=None):
    """dt_conv32x_split on samples pool[a] with the pool's in_eps.  Returns (y:
    int16 [n, image] for layers 2 / 3, float32 [n, 4032] for conv4; part)."""
    n = a.shape[0]
    last = layer == 4
    x = (_mix('xin', p, a, p2, n0) if xin is None else xin).contiguous()
    if prev is None:
        prev = _mix('prev', p, a, p2, n0).contiguous()
    if last:
        ywhole, y = _canary(n * 4032, torch.float32, gpu)
        pwhole, part = None, None
    else:
        ywhole, y = _canary(n * _hlb_elems(layer), torch.float16, gpu)
        pwhole, part = _canary(n * 96, torch.float32, gpu)
    rc = _lib().dt_conv32x_split(
        layer, n, x.data_ptr(), (p['wf'] if wf is None else wf).data_ptr(), p['b'].data_ptr(),
        prev.data_ptr(), p['gamma'].data_ptr(), p['beta'].data_ptr(), p['eps'], y.data_ptr(),
        _ptr(part), p['og'].data_ptr() if last else None, p['ob'].data_ptr() if last else None,
        X.EPS if last else 0.0, X.SLOPE, _split(n0, p2, layer) if p2 else None, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    _tail_untouched(ywhole, y.numel())
    if last:
        return y.view(n, 4032), None
    _tail_untouched(pwhole, part.numel())
    return y.view(torch.int16).view(n, -1), part.view(n, 32, 3)


def _out4_bad(y, want, unit):
    """conv4's normalised output against float64: the elements over the bound
    [n, 4032] (bool) and the worst error / bound."""
    bound = X.K_OUT4 * X.U * unit
    err = (y.double() - want).abs()
    return err > bound, (err / bound).max().item()


def _sets(p, p2, n0, n):
    return ((p, slice(0, n0)), (p2, slice(n0, n))) if p2 else ((p, slice(0, n)),)


def _check(layer, y, part, p, a, what, p2=None, n0=None):
    """Layers 1..3: the HLB image and the centres equal, the statistics within
    their bounds; conv4: the normalised output within its bound, exactly
    out_beta in the channels without weights."""
    n = a.shape[0]
    if layer == 4:
        assert bool(torch.isfinite(y).all()), what
        bad, worst = _out4_bad(y, _mix('want', p, a, p2, n0), _mix('unit', p, a, p2, n0))
        print('%s: normalised output error / bound %.3f' % (what, worst))
        assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[0].tolist(), worst)
        for q, sl in _sets(p, p2, n0, n):
            for co in X.ZERO_CO:
                got = y.view(n, 32, -1)[sl, co]
                assert bool((got == q['ob'][co]).all()), (what, co)
        return
    _first_diff(y, _mix('img', p, a, p2, n0), what + ' (hi, lo) image')
    want_part = _mix('part', p, a, p2, n0)
    _first_diff(part[..., 2].contiguous().view(torch.int32),
                want_part[..., 2].float().contiguous().view(torch.int32), what + ' centre')
    for q, sl in _sets(p, p2, n0, n):
        _stats_ok(part[sl], q, a[sl].to(part.device), layer, what)
    for co in X.ZERO_CO:             # zero weights: (0, 0, c) exactly
        assert bool((part[:, co, :2] == 0).all()), (what, co)


@pytest.mark.parametrize('slots,order', [(4, [2, 3, 0]), (3, [1, 0, 2])])
@pytest.mark.parametrize('count', COUNTS)
def test_conv1x_is_exact(gpu, count, slots, order):
    """conv1 from the grey f32 ring: every stored (hi, lo) pair and centre
    equal, (mean, M2) within four times the float32 restatement."""
    n = _count(count, gpu)
    p, a = _pool(gpu, 1), _picks(n, 1)
    y, part = _run1x(gpu, p, a, slots, order)
    _check(1, y, part, p, a, 'conv1x n=%d' % n)


@pytest.mark.parametrize('var', ['plain', 'eps'])
@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('layer', [2, 3, 4])
def test_conv32x_is_exact(gpu, layer, count, var):
    """conv2..conv4 per layer with the previous BatchNorm folded into the
    weights (in_eps = 0) and the flat-channel variant (in_eps = 1e-5, the flat
    channel's weights non-zero in every tap: it must contribute exactly sum w
    beta).  Layers 2 / 3: bits equal; conv4: its own BatchNorm's f32 output
    within the derived bound, out_beta exactly in the channels without weights."""
    n = _count(count, gpu)
    p, a = _pool(gpu, layer, 0, var), _picks(n, layer)
    y, part = _run32x(gpu, layer, p, a)
    _check(layer, y, part, p, a, 'conv%dx %s n=%d' % (layer, var, n))


@pytest.mark.parametrize('case', ['n3-n0=1', 'n3-n0=2', 'big-n0=1', 'big-n0=n-1', 'big-n0=n/3'])
@pytest.mark.parametrize('layer', [1, 2, 3, 4])
def test_two_weight_sets_are_exact_x3(gpu, layer, case):
    """One launch over two exact weight sets: every sample gets the
    expectation of its own set, with the split after the first sample, before
    the last and inside the range."""
    n = 3 if case.startswith('n3') else _count('5cu/2+3', gpu)
    n0 = {'n3-n0=1': 1, 'n3-n0=2': 2, 'big-n0=1': 1, 'big-n0=n-1': n - 1, 'big-n0=n/3': n // 3}[case]
    p, p2 = _pool(gpu, layer, 0), _pool(gpu, layer, 1)
    a = _picks(n, 10 + layer)
    what = 'conv%dx split n=%d n0=%d' % (layer, n, n0)
    if layer == 1:
        y, part = _run1x(gpu, p, a, 3, [2, 0, 1], p2, n0)
    else:
        y, part = _run32x(gpu, layer, p, a, p2, n0)
    _check(layer, y, part, p, a, what, p2, n0)


@pytest.mark.parametrize('var', ['rescale', 'subw', 'sublo'])
@pytest.mark.parametrize('layer', [2, 3, 4])
def test_rare_fold_branches_are_exact(gpu, layer, var):
    """The fold's power-of-two rescale (e = 2 in six pool samples and 0 in the
    seventh of the same launch: the scale is per sample), folded weights whose
    hi half is an fp16 subnormal, inputs whose lo halves are fp16 subnormals:
    the expectation is the exact model in each."""
    n = 19
    p, a = _pool(gpu, layer, 0, var), _picks(n, 40 + layer)
    if var == 'rescale':
        a[5] = X.RS_OFF                  # a sample without the rescale among those with it
        assert (a != X.RS_OFF).any()
    y, part = _run32x(gpu, layer, p, a)
    _check(layer, y, part, p, a, 'conv%dx %s n=%d' % (layer, var, n))


@pytest.mark.parametrize('n', [1, 3, 19])
def test_index_ring_gives_the_grey_rings_bits(gpu, n):
    """A palette-index ring gives conv1x the bits its decoded grey ring
    gives: image, centres and statistics, slots that `order` skips differing."""
    from aido1_amd.render import decode_index
    p = _pool(gpu, 1)
    g = torch.Generator(device=gpu).manual_seed(n)
    idx = torch.randint(0, 8, (n, 4, 120, 160), dtype=torch.uint8, device=gpu, generator=g)
    order = [3, 1, 2]
    grey = decode_index(idx).float().contiguous()
    grey[:, 0] = float('nan')
    yi, pi = _launch1x(gpu, idx, True, order, p['wf'], p['b'], None)
    yg, pg = _launch1x(gpu, grey, False, order, p['wf'], p['b'], None)
    _first_diff(yi, yg, 'index / grey image')
    _first_diff(pi.contiguous().view(torch.int32), pg.contiguous().view(torch.int32),
                'index / grey part')
    assert bool(torch.isfinite(pi).all())


@pytest.mark.parametrize('layer', [2, 3, 4])
def test_one_lo_grain_of_one_tap_is_noticed(gpu, layer):
    """Sensitivity (a): one tap of one (co, ci) pair raised by one grain of
    its lo half (2^-13; 1e-5 max(1, max|ref|) is a thousand times that).
    Layers 2 / 3: the image equals the perturbed expectation bit for bit and
    differs from the unperturbed one in channel co alone.  conv4: against the
    unperturbed launch every other channel keeps its bits, channel co does
    not, and the output is within the bound of the perturbed expectation."""
    n, co = 19, 9
    from aido1_amd.actor import conv32_fragments
    p, a = _pool(gpu, layer), _picks(n, 20 + layer)
    src = X.pool32x(layer, 0, 'plain')
    w, v, _ = X.perturbed_tap(src, co=co)
    wf = conv32_fragments(w.to(gpu), torch.float32).contiguous()
    y, part = _run32x(gpu, layer, p, a, wf=wf)
    ag = a.to(gpu)
    if layer == 4:
        y0, _ = _run32x(gpu, layer, p, a)
        same = (y.view(torch.int32) == y0.view(torch.int32)).view(n, 32, -1)
        assert not bool(same[:, co].all()), 'the moved tap left channel %d unchanged' % co
        same[:, co] = True
        assert bool(same.all()), 'changes outside channel %d' % co
        vf = v.flatten(2)
        mu, mm = R._stats64(vf)
        s64 = src['og'].double() / torch.sqrt(mm / vf.shape[-1] + X.EPS)
        want = ((vf - mu[..., None]) * s64[..., None] + src['ob'].double()[..., None]).flatten(1)
        bad, worst = _out4_bad(y, want.to(gpu)[ag], p['unit'][ag])
        assert not bool(bad.any()), worst
        return
    d32 = (v - v[:, :, :1, :1]).permute(0, 2, 3, 1).float().contiguous().to(gpu)
    img = X.hlb_image(d32, X.NEXT_STRIDE[layer], S16)
    _first_diff(y, img.flatten(1)[ag], 'conv%dx moved tap' % layer)
    oh, ow, _ = _out_geom(layer)
    diff = (y != p['img'][ag]).view(n, oh, 4, 2, -1, 8)      # block cb holds channels 8 cb .. + 7
    assert bool(diff[:, :, co // 8, :, :, co % 8].any()), 'the expectation missed the moved tap'
    diff[:, :, co // 8, :, :, co % 8] = False
    assert not bool(diff.any()), 'mismatches outside channel %d' % co


def test_swapped_weight_halves_of_one_k_step_are_noticed_conv1x(gpu):
    """Sensitivity (b): the hi and lo fragments of conv1's k step 5 swapped
    before the launch: the image no longer equals the expectation."""
    n = 19
    p, a = _pool(gpu, 1), _picks(n, 50)
    wf = p['wf'].clone()
    wf[:, 5] = wf[[1, 0], 5]
    assert not torch.equal(wf, p['wf'])
    y, _ = _run1x(gpu, p, a, 3, [0, 1, 2], wf=wf)
    bad = (y != p['img'][a.to(gpu)]).any(1)
    assert bool(bad.all()), 'swapped (hi, lo) fragments passed in %d samples' % int((~bad).sum())


@pytest.mark.parametrize('layer', [2, 3, 4])
def test_swapped_input_halves_are_noticed(gpu, layer):
    """Sensitivity (b): the hi and lo segments of one channel block of one
    input row of one sample swapped (a k step's B fragments): mismatches in
    that sample and no other."""
    n, i = 19, 4
    p, a = _pool(gpu, layer), _picks(n, 60 + layer)
    ih = X.GEOM[layer][0]
    xin = _mix('xin', p, a).clone().view(n, ih, 4, 2, -1, 8)
    xin[i, 3, 1] = xin[i, 3, 1].flip(0)
    y, part = _run32x(gpu, layer, p, a, xin=xin.view(n, -1))
    ag = a.to(gpu)
    if layer == 4:
        bad, _ = _out4_bad(y, p['want'][ag], p['unit'][ag])
    else:
        bad = y != p['img'][ag]
    assert bad.any(1).nonzero().flatten().tolist() == [i]


@pytest.mark.parametrize('layer', [2, 3, 4])
def test_swapped_statistics_are_noticed_x3(gpu, layer):
    """Sensitivity (c): two samples' prev_part rows swapped before the launch
    (a sample folded with its neighbour's statistics): mismatches in exactly
    those two samples (conv4: elements over its bound)."""
    n, i = 19, 3
    p, a = _pool(gpu, layer), _picks(n, 30 + layer)
    j = next(k for k in range(i + 1, n) if a[k] != a[i])
    prev = _mix('prev', p, a).clone()
    prev[[i, j]] = prev[[j, i]]
    y, part = _run32x(gpu, layer, p, a, prev=prev.contiguous())
    ag = a.to(gpu)
    if layer == 4:
        bad, _ = _out4_bad(y, p['want'][ag], p['unit'][ag])
    else:
        bad = y != p['img'][ag]
    assert bad.any(1).nonzero().flatten().tolist() == [i, j]


def _pair_value(y, layer, n):
    """The (hi, lo) image [n, image] (int16) -> hi + 2^-11 lo, float64 NCHW."""
    from aido1_amd.actor import hlb_decode
    oh, ow, sn = _out_geom(layer)
    return hlb_decode(y.view(torch.float16), oh, ow, sn).permute(0, 3, 1, 2)


@pytest.mark.parametrize('layer', [1, 2, 3, 4])
def test_real_valued_inputs_within_the_elementwise_bound_x3(gpu, layer):
    """Realistic inputs at n = 19 (conv2..4: test_gpu_actor_x3._layer_case,
    per-channel spreads e^(2 N(0,1)), in_eps = 1e-5; conv1: uniform frames)
    against float64, elementwise, with w' = w sc the folded weights and x the
    values the kernel reads:

      |v_kernel - v| <= K 2^-24 (|w'| * |x|) + 2^-22 |v - c|,
      K = 512 + 8 (conv2..4: 512 float32 accumulations, 8 for sc, sh, the
      operands' own 2^-24 and the dropped lo products), 192 + 8 (conv1)

    the second term for the pair store.  conv4's own BatchNorm carries that
    bound e through its normalisation as the fp16 file does: with s =
    sqrt(var + eps), s' = s - rms(e),

      |err| <= gamma ((e + mean e) / s' + |v - mean| rms(e) / (s s'))
               + K_OUT4 u (|v| sc + mean|v| sc + |out_beta|)."""
    from aido1_amd.actor import conv1_fragments, conv32_fragments, hlb_decode, split_hl
    from test_gpu_actor_x3 import _layer_case
    n = 19
    ih, iw, oh, ow, st, _ = X.GEOM[layer]
    slope = 0.01
    s32 = float(np.float32(slope))
    g = torch.Generator(device=gpu).manual_seed(200 + layer)
    if layer == 1:
        ring = torch.rand(n, 3, 120, 160, device=gpu, generator=g)
        w = torch.randn(32, 3, 8, 8, device=gpu, generator=g) * 0.08
        b = torch.randn(32, device=gpu, generator=g) * 0.2
        acc = F.conv2d(ring.double(), w.double(), b.double(), stride=2)
        e = (192 + 8) * X.U * F.conv2d(ring.double(), w.double().abs(), stride=2)
        wf = split_hl(conv1_fragments(w, torch.float32)).contiguous()
        ywhole, y = _canary(n * _hlb_elems(1), torch.float16, gpu)
        pwhole, part = _canary(n * 96, torch.float32, gpu)
        rc = _lib().dt_conv1x_split(ring.data_ptr(), 0, n, 3, (ctypes.c_int32 * 3)(0, 1, 2),
                                    wf.data_ptr(), b.data_ptr(), None, y.data_ptr(),
                                    part.data_ptr(), slope, _stream())
    else:
        xh, prev, gamma, beta, w, b, _ = _layer_case(gpu, layer, n, 300 + layer)
        xt = hlb_decode(xh, ih, iw, st)
        pm, pv = prev[..., 0].double(), prev[..., 1].double() / (ih * iw)
        sc = gamma.double() / torch.sqrt(pv + X.EPS)
        xn = ((xt - pm[:, None, None, :]) * sc[:, None, None, :] + beta.double()).permute(0, 3, 1, 2)
        acc = F.conv2d(xn, w.double(), b.double(), stride=st)
        e = (512 + 8) * X.U * F.conv2d((xt * sc[:, None, None, :]).abs().permute(0, 3, 1, 2),
                                       w.double().abs(), stride=st)
        og = torch.rand(32, device=gpu, generator=g) + 0.5
        ob = torch.rand(32, device=gpu, generator=g) - 0.5
        last = layer == 4
        wf = conv32_fragments(w, torch.float32).contiguous()
        if last:
            ywhole, y = _canary(n * 4032, torch.float32, gpu)
            pwhole, part = None, None
        else:
            ywhole, y = _canary(n * _hlb_elems(layer), torch.float16, gpu)
            pwhole, part = _canary(n * 96, torch.float32, gpu)
        rc = _lib().dt_conv32x_split(layer, n, xh.data_ptr(), wf.data_ptr(), b.data_ptr(),
                                     prev.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-5,
                                     y.data_ptr(), _ptr(part), og.data_ptr() if last else None,
                                     ob.data_ptr() if last else None, 1e-5 if last else 0.0,
                                     slope, None, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    v = torch.maximum(acc, acc * s32)
    _tail_untouched(ywhole, y.numel())
    assert bool(torch.isfinite(y).all())
    if layer == 4:
        vf, ef = v.flatten(2), e.flatten(2)
        mu = vf.mean(-1, keepdim=True)
        s = torch.sqrt(((vf - mu) ** 2).mean(-1, keepdim=True) + X.EPS)
        s_lo = s - torch.sqrt((ef ** 2).mean(-1, keepdim=True))
        assert bool((s_lo > 0.5 * s).all())
        gd, bd = og.double().view(1, 32, 1), ob.double().view(1, 32, 1)
        want = (vf - mu) / s * gd + bd
        unit = (vf.abs() + vf.abs().mean(-1, keepdim=True)) * gd / s + bd.abs()
        bound = gd * ((ef + ef.mean(-1, keepdim=True)) / s_lo +
                      (vf - mu).abs() * (s - s_lo) / (s * s_lo)) + X.K_OUT4 * X.U * unit
        err = (y.view(n, 32, oh * ow).double() - want).abs()
    else:
        _tail_untouched(pwhole, part.numel())
        c = part.view(n, 32, 3)[..., 2].double()
        assert bool(((c - v[:, :, 0, 0]).abs() <= e[:, :, 0, 0]).all())
        got = _pair_value(y.view(torch.int16).view(n, -1), layer, n) + c[:, :, None, None]
        bound = e + 2.0 ** -22 * (v - v[:, :, :1, :1]).abs()
        err = (got - v).abs()
    print('conv%dx real-valued: worst error / bound %.3f' % (layer, (err / bound).max().item()))
    assert bool((err <= bound).all()), (int((err > bound).sum()), (err / bound).max().item())


def _head_pool(gpu, seed):
    """pool_head on the device with lin1's (hi, lo) fragments, built as the
    actor's refresh builds them (the head index map, then split_hl)."""
    from aido1_amd.actor import head_fragment_index, split_hl
    key = ('head', seed)
    if key not in _DEV:
        src = X.pool_head(seed)
        p = {k: src[k].to(gpu) for k in ('x', 'w1', 'b1', 'w2', 'b2', 'parts', 'out')}
        p['w1x'] = split_hl(torch.take(p['w1'], head_fragment_index(gpu))).contiguous()
        _DEV[key] = p
    return _DEV[key]


def _run_head(gpu, n, n0, pa, pb, a, w1x=None):
    x = _mix('x', pa, a, pb, n0).contiguous()
    wwhole, work = _canary(int(_lib().dt_actor_head_x3_work_floats(n)), torch.float32, gpu)
    owhole, out = _canary(2 * n, torch.float32, gpu)
    sec = [pb[k].data_ptr() for k in ('w1x', 'b1', 'w2', 'b2')] if pb else [None] * 4
    rc = _lib().dt_actor_head_x3(n, n0, 4032, x.data_ptr(),
                                 (pa['w1x'] if w1x is None else w1x).data_ptr(), pa['b1'].data_ptr(),
                                 pa['w2'].data_ptr(), pa['b2'].data_ptr(), *sec, 0, X.SLOPE,
                                 work.data_ptr(), out.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    _tail_untouched(wwhole, work.numel())
    _tail_untouched(owhole, out.numel())
    return work.view(4, 512, n), out.view(n, 2)


def _head_want(pa, pb, a, n0):
    ag = a.to(pa['out'].device)
    out = _mix('out', pa, a, pb, n0).float()
    parts = pa['parts'][:, :, ag]
    if pb is not None:
        parts = torch.cat([parts[:, :, :n0], pb['parts'][:, :, ag[n0:]]], 2)
    return parts.float().contiguous(), out.contiguous()


@pytest.mark.parametrize('n,n0', HEAD_CASES)
def test_head_lin1_is_exact(gpu, n, n0):
    """dt_actor_head_x3 at head code 0 on dyadic inputs with lo != 0 in x and
    in lin1's weights, two weight sets where n0 < n: lin1's partial sums of
    the four K quarters (the work buffer, [4][512][n]) and the output [n, 2]
    equal the float64 model bit for bit."""
    pa = _head_pool(gpu, 0)
    pb = _head_pool(gpu, 1) if n0 < n else None
    a = _picks(n, 70 + n0)
    work, out = _run_head(gpu, n, n0, pa, pb, a)
    want_parts, want_out = _head_want(pa, pb, a, n0)
    _first_diff(work.permute(2, 0, 1).contiguous().view(torch.int32),
                want_parts.permute(2, 0, 1).contiguous().view(torch.int32),
                'head n=%d n0=%d lin1 partial sums [sample][quarter, feature]' % (n, n0))
    _first_diff(out.contiguous().view(torch.int32), want_out.view(torch.int32),
                'head n=%d n0=%d output' % (n, n0))


def test_swapped_lin1_halves_of_one_k_step_are_noticed(gpu):
    """Sensitivity (b) for the head: the hi and lo fragments of lin1's k step
    100 (K quarter 1) swapped: that quarter's partial sums differ in every
    sample, the other quarters keep their bits."""
    n = 33
    pa, a = _head_pool(gpu, 0), _picks(n, 80)
    w1x = pa['w1x'].clone().view(2, 16, 252, 64, 8)
    w1x[:, :, 100] = w1x[[1, 0]][:, :, 100]
    work, _ = _run_head(gpu, n, n, pa, None, a, w1x=w1x.view_as(pa['w1x']).contiguous())
    want_parts, _ = _head_want(pa, None, a, n)
    diff = work.contiguous().view(torch.int32) != want_parts.view(torch.int32)
    assert bool(diff[1].any(0).all()), 'swapped lin1 fragments passed'
    diff[1] = False
    assert not bool(diff.any())
