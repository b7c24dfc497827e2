"""The three GPU Canny implementations against tests/canny_ref.py, bit for bit:
line_detect_kernel (images in LDS), line_detect_big_kernel (a device
workspace) and the render kernel's listed-word Canny.  Not against the C
oracle, from which all three descend: canny_ref is a second, differently
built statement of the algorithm, and tests/test_canny_ref.py shows that
agreeing with it on these inputs excludes each of its listed near-misses."""
import numpy as np
import pytest
import torch

import canny_ref as C
from test_gpu_render_masks import _env, _jitter

pytestmark = pytest.mark.gpu


def _check_line_detect(gpu, named):
    """One launch per threshold pair and hsv flag over the images `named`
    ([(name, image)], one size): plane 3 is canny_ref's map of each image,
    with and without the HSV output."""
    from aido1_amd.render import LineParams, line_detect
    assert len(named) > 1
    batch = np.stack([img for _, img in named])
    dev = torch.from_numpy(batch).to(gpu)
    for lo, hi in C.THRESHOLDS:
        lp = LineParams.default()
        lp.canny_lo, lp.canny_hi = lo, hi
        plain = line_detect(dev, lp)[:, 3].cpu().numpy()
        with_hsv = line_detect(dev, lp, hsv=True)[0][:, 3].cpu().numpy()
        assert np.array_equal(plain, with_hsv), (lo, hi)
        assert np.isin(plain, (0, 255)).all()
        for (name, img), got in zip(named, plain > 0):
            assert np.array_equal(got, C.canny_ref(img, lo, hi)), (name, img.shape[:2], lo, hi)


@pytest.mark.parametrize('shape', C.SIZES)
def test_line_detect_lds_fixtures(gpu, shape):
    """Every fixture image of one size in one launch (different images in one
    grid), at every threshold pair."""
    _check_line_detect(gpu, C.images(*shape))


def test_line_detect_lds_full_image(gpu):
    """120 x 160, all the LDS image holds: noise, ties, and the serpentine, whose
    weak chain takes thousands of hysteresis sweeps to follow."""
    rng = np.random.default_rng(120160)
    _check_line_detect(gpu, [('noise', C.noise(rng, 120, 160)),
                             ('quantised_grey', C.quantised_grey(rng, 120, 160)),
                             ('serpentine', C.serpentine(120, 160))])


def test_line_detect_workspace_stride(gpu):
    """121 x 161 = 19,481 pixels, just past the LDS image and no multiple of
    256: three images, each at its own rounded-up workspace offset."""
    from aido1_amd import _lib
    h, w = 121, 161
    assert _lib.lib().dt_line_detect_workspace(3, h, w) > 0 and (h * w) % 256
    rng = np.random.default_rng(121161)
    _check_line_detect(gpu, [('noise', C.noise(rng, h, w)),
                             ('quantised_grey', C.quantised_grey(rng, h, w)),
                             ('staircase', C.staircase(h, w))])


def test_line_detect_workspace_one_row(gpu):
    """1 x 19201: every gradient is horizontal, every vertical neighbour is
    outside the image."""
    rng = np.random.default_rng(19201)
    _check_line_detect(gpu, [('noise', C.noise(rng, 1, 19201)),
                             ('quantised', C.quantised(rng, 1, 19201))])


def test_line_detect_workspace_serpentine(gpu):
    """150 x 200 through the workspace: noise, and the deeper serpentine over
    the listed weak candidates in device memory."""
    rng = np.random.default_rng(150200)
    _check_line_detect(gpu, [('noise', C.noise(rng, 150, 200)),
                             ('serpentine', C.serpentine(150, 200))])


def _render(gpu, map_name, lo, hi, list_cap):
    """(rgb, edge planes) of 32 jittered spawn poses from the render kernel."""
    from aido1_amd.render import LineParams, RenderOutput
    n = 32
    env = _env(map_name, n, seed=41)
    x, z, a = _jitter(env.get_state(), np.random.default_rng(42))
    env.set_state(x=x, z=z, angle=a)
    lp = LineParams.default()
    lp.canny_lo, lp.canny_hi = lo, hi
    env.set_line_params(lp)
    out = RenderOutput(n, gpu, slots=1, rgb=True)
    env.render_into(out, list_cap=list_cap)
    torch.cuda.synchronize()
    return out.rgb.cpu().numpy(), out.masks[:, 3].cpu().numpy() > 0


@pytest.mark.parametrize('map_name', ['loop_empty', 'zigzag'])
def test_render_canny_default_thresholds(gpu, map_name):
    rgb, edges = _render(gpu, map_name, 80.0, 200.0, 0)
    assert edges.any()
    for i in range(len(rgb)):
        assert np.array_equal(edges[i], C.canny_ref(rgb[i, ..., ::-1], 80.0, 200.0)), i


@pytest.mark.parametrize('list_cap', [0, 64])
@pytest.mark.parametrize('map_name', ['loop_empty', 'zigzag'])
def test_render_canny_weak_lists(gpu, map_name, list_cap):
    """20 / 1200: most candidates are weak.  By the reference, some frames
    have more weak candidates than the kernel's weak list holds (512: the
    hysteresis then walks every listed word) and some have 1 .. 512 (it walks
    the list); with the default word list and with list_cap = 64 (the spill)."""
    lo, hi = 20.0, 1200.0
    rgb, edges = _render(gpu, map_name, lo, hi, list_cap)
    n_weak = []
    for i in range(len(rgb)):
        cand, strong, ref = C.canny_parts(rgb[i, ..., ::-1], lo, hi)
        n_weak.append(int((cand & ~strong).sum()))
        assert np.array_equal(edges[i], ref), i
    n_weak = np.array(n_weak)
    over, listed = int((n_weak > 512).sum()), int(((n_weak > 0) & (n_weak <= 512)).sum())
    print('%s: %d frames past the weak list, %d within it' % (map_name, over, listed))
    assert over > 0 and listed > 0
