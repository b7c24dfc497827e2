"""The Canny edge map (mask plane 3) against an independent restatement.

tests/canny_ref.py states cv2.Canny's rules (apertureSize 3, L1 gradient, a
3-channel 8-bit image) a second time, structured differently from
oracle/render_oracle.c on purpose.  Here, on the CPU: its floating-point
sector rule is cv2's fixed-point one for every possible gradient; the C
oracle's edge plane equals it on every fixture; every listed near-miss (one
rule changed) differs from it on at least one fixture, so agreement on the
fixtures excludes those mistakes; and the serpentines are as deep as the
GPU hysteresis tests need them.  tests/test_gpu_canny.py holds the kernels to
the same reference on the same inputs.  (cv2 is absent: parity with an OpenCV
binary stays unchecked.)"""
import math

import numpy as np
import pytest

import canny_ref as C
from conftest import map_rows
from oracle import oracle_c as OC


def oracle_edges(img, lo, hi, _cache={}):
    if (lo, hi) not in _cache:
        p = OC.line_params_default()
        p.canny_lo, p.canny_hi = lo, hi
        _cache[lo, hi] = OC.OracleRender(map_rows('loop_empty'), params=p)
    return _cache[lo, hi].line_detect(img[None])[0, 3] > 0


@pytest.fixture(scope='module')
def refs():
    """[(name, image, lo, hi, canny_ref's edge map)], computed once."""
    return [(name, img, lo, hi, C.canny_ref(img, lo, hi)) for name, img, lo, hi in C.cases()]


@pytest.fixture(scope='module')
def serpentines():
    out = {}
    for h, w in ((120, 160), (150, 200)):
        img = C.serpentine(h, w)
        out[h, w] = (img,) + C.canny_parts(img, 80.0, 200.0)
    return out


def test_sector_rule_is_cv2s_fixed_point_rule():
    """The angle test in floating point (tan 22.5 = sqrt 2 - 1, tan 67.5 =
    sqrt 2 + 1) and cv2's 15-bit fixed-point test give the same sector for
    every |gx|, |gy| a 3 x 3 Sobel of 8-bit data can produce (0 .. 1020)."""
    ax, ay = np.meshgrid(np.arange(1021), np.arange(1021), indexing='ij')
    h, v = C.sectors(ax, ay)
    ch, cv = C.sectors_cv2(ax, ay)
    assert np.array_equal(h, ch) and np.array_equal(v, cv)
    assert h.any() and v.any() and (~h & ~v).any()


def test_fixture_families(refs):
    """The families are what the module says: every size, every threshold
    pair, the staircase's magnitudes, edges in most cases and none in some."""
    assert {i.shape[:2] for _, i, _, _, _ in refs} == set(C.SIZES)
    assert {(lo, hi) for _, _, lo, hi, _ in refs} == set(C.THRESHOLDS)
    assert any(lo > hi for lo, hi in C.THRESHOLDS) and any(lo == hi for lo, hi in C.THRESHOLDS)
    assert any(lo != math.floor(lo) for lo, _ in C.THRESHOLDS)
    # the staircase's magnitude-120 pixels: weak edges at lo = 119.6, nothing at lo = 120
    cand, strong, edges = C.canny_parts(C.staircase(24, 40), 119.6, 200.0)
    at120 = C.canny_ref(C.staircase(24, 40), 120.0, 200.0)
    assert strong.any() and np.array_equal(cand, edges) and at120[strong].all()
    assert (edges & ~at120).sum() >= 8 and not (at120 & ~edges).any()
    n_edges = [int(e.sum()) for *_, e in refs]
    assert sum(k > 0 for k in n_edges) > len(refs) // 2 and 0 in n_edges


def test_oracle_equals_canny_ref_on_fixtures(refs):
    for name, img, lo, hi, ref in refs:
        assert np.array_equal(oracle_edges(img, lo, hi), ref), name


@pytest.mark.parametrize('mutant', C.MUTANTS)
def test_mutant_is_killed(refs, mutant):
    """One rule changed gives another edge map on at least one fixture."""
    assert any(not np.array_equal(C.canny_ref(img, lo, hi, mutant), ref)
               for _, img, lo, hi, ref in refs), mutant


@pytest.mark.parametrize('shape,floor', [((120, 160), 2000), ((150, 200), 3000)])
def test_serpentine_depth(serpentines, shape, floor):
    """Few strong pixels, and the weak edge pixel farthest from them is
    thousands of 8-connected steps away: a hysteresis that stops early (a
    sweep cap, a lost `changed` flag, a stale read) leaves edges out."""
    img, cand, strong, edges = serpentines[shape]
    assert 0 < strong.sum() <= 16
    assert np.array_equal(cand, edges)            # one component: all of it is found
    depth = C.hysteresis_depth(strong, edges)
    print('serpentine %dx%d: %d strong, %d edges, depth %d'
          % (shape + (strong.sum(), edges.sum(), depth)))
    assert depth >= floor
    assert np.array_equal(oracle_edges(img, 80.0, 200.0), edges)
    # and the chain is what makes them edges: without hysteresis only the patch is
    assert C.canny_ref(img, 80.0, 200.0, 'no_hysteresis').sum() == strong.sum()


@pytest.mark.parametrize('lo,hi', [(80.0, 200.0), (20.0, 1200.0)])
@pytest.mark.parametrize('map_name', ['loop_empty', 'zigzag'])
def test_oracle_equals_canny_ref_on_rendered_frames(map_name, lo, hi):
    """The oracle's own frames (flat colours, Bresenham markings): its edge
    plane is canny_ref of its raster, 32 seeded poses a map."""
    n = 32
    rng = np.random.default_rng(len(map_name) + int(hi))
    ts = 0.61
    x, z = rng.uniform(0, 3 * ts, n), rng.uniform(0, 3 * ts, n)
    a = rng.uniform(-math.pi, math.pi, n)
    p = OC.line_params_default()
    p.canny_lo, p.canny_hi = lo, hi
    _, masks, rgb = OC.OracleRender(map_rows(map_name), params=p).render(x, z, a)
    assert (masks[:, 3] > 0).any()
    for i in range(n):
        assert np.array_equal(masks[i, 3] > 0, C.canny_ref(rgb[i, ..., ::-1], lo, hi)), i
