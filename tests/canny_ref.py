"""An independent statement of the Canny edge map, and inputs that tell it
from its near-misses.

canny_ref restates cv2.Canny(bgr, lo, hi, apertureSize=3, L2gradient=False)
for one 3-channel 8-bit image from the published rules, in whole-image
numpy / scipy operations: scipy's correlate for the Sobel pair, argmax for the
channel choice, a floating-point angle test for the sector, shifted views of
a zero-padded magnitude plane for non-maximum suppression, and connected
component labelling for hysteresis.  It shares no code and no structure with
oracle/render_oracle.c (a per-pixel loop, fixed-point sectors, a stack flood
fill) or with the kernels pinned to it.

Each name in MUTANTS changes one rule.  cases() lists the (image, lo, hi)
inputs the tests run; tests/test_canny_ref.py asserts that every mutant
differs from canny_ref on at least one of them, so an implementation that
agrees with canny_ref on all of them has none of those mistakes.
"""
import math

import numpy as np
from scipy import ndimage

SOBEL_X = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.int64)
SOBEL_Y = SOBEL_X.T.copy()
EIGHT = np.ones((3, 3), bool)
FOUR = ndimage.generate_binary_structure(2, 1)

MUTANTS = (
    'no_swap',            # lo > hi left as given
    'round_thresholds',   # floor -> round half up
    'ceil_thresholds',    # floor -> ceil
    'sobel_mirror',       # BORDER_REPLICATE -> BORDER_REFLECT_101
    'sobel_zero',         # BORDER_REPLICATE -> zero border
    'l2_magnitude',       # |gx| + |gy| -> sqrt(gx^2 + gy^2)
    'last_channel',       # first maximum channel -> last
    'channel0',           # maximum channel -> channel 0
    'mag_replicate',      # magnitude outside the image: 0 -> replicated
    'sector_half_two',    # tan 22.5 / tan 67.5 -> 0.5 / 2.0
    'diag_flip',          # the two diagonals exchanged
    'second_gt',          # horizontal / vertical: m >= second -> m > second
    'first_ge',           # horizontal / vertical: m > first -> m >= first
    'diag_ge',            # diagonal: m > both -> m >= both
    'lo_ge',              # m > lo -> m >= lo
    'hi_ge',              # m > hi -> m >= hi
    'conn4',              # 8-connected hysteresis -> 4-connected
    'no_hysteresis',      # strong pixels only
)

T22 = math.sqrt(2.0) - 1.0   # tan 22.5 deg
T67 = math.sqrt(2.0) + 1.0   # tan 67.5 deg


def thresholds(lo, hi, mutant=None):
    if lo > hi and mutant != 'no_swap':
        lo, hi = hi, lo
    if mutant == 'round_thresholds':
        return math.floor(lo + 0.5), math.floor(hi + 0.5)
    if mutant == 'ceil_thresholds':
        return math.ceil(lo), math.ceil(hi)
    return math.floor(lo), math.floor(hi)


def sectors(ax, ay, mutant=None):
    """(horizontal, vertical) of gradients |gx| = ax, |gy| = ay; the rest is
    diagonal.  By the angle, in floating point."""
    t_lo, t_hi = (0.5, 2.0) if mutant == 'sector_half_two' else (T22, T67)
    ax, ay = ax.astype(np.float64), ay.astype(np.float64)
    horizontal = ay < t_lo * ax
    vertical = ~horizontal & (ay > t_hi * ax)
    return horizontal, vertical


def sectors_cv2(ax, ay):
    """cv2's fixed-point rule (TG22 = 13573 = round(tan 22.5 * 2^15))."""
    ax, ay = ax.astype(np.int64), ay.astype(np.int64)
    tg22x = ax * 13573
    horizontal = (ay << 15) < tg22x
    vertical = ~horizontal & ((ay << 15) > tg22x + (ax << 16))
    return horizontal, vertical


def canny_parts(bgr, lo, hi, mutant=None):
    """(candidates, strong, edges), bool [h, w] each."""
    assert mutant is None or mutant in MUTANTS, mutant
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
    h, w, _ = bgr.shape
    lo, hi = thresholds(lo, hi, mutant)

    mode = {'sobel_mirror': 'mirror', 'sobel_zero': 'constant'}.get(mutant, 'nearest')
    planes = bgr.astype(np.int64).transpose(2, 0, 1)
    gx3 = np.stack([ndimage.correlate(p, SOBEL_X, mode=mode, cval=0) for p in planes])
    gy3 = np.stack([ndimage.correlate(p, SOBEL_Y, mode=mode, cval=0) for p in planes])
    if mutant == 'l2_magnitude':
        m3 = np.sqrt((gx3 * gx3 + gy3 * gy3).astype(np.float64))
    else:
        m3 = np.abs(gx3) + np.abs(gy3)

    if mutant == 'channel0':
        ch = np.zeros((h, w), np.int64)
    elif mutant == 'last_channel':
        ch = 2 - np.argmax(m3[::-1], axis=0)
    else:
        ch = np.argmax(m3, axis=0)
    pick = ch[None]
    gx = np.take_along_axis(gx3, pick, 0)[0]
    gy = np.take_along_axis(gy3, pick, 0)[0]
    m = np.take_along_axis(m3, pick, 0)[0]

    horizontal, vertical = sectors(np.abs(gx), np.abs(gy), mutant)
    same_sign = (gx < 0) == (gy < 0)
    if mutant == 'diag_flip':
        same_sign = ~same_sign

    if mutant == 'mag_replicate':
        mp = np.pad(m, 1, mode='edge')
    else:
        mp = np.pad(m, 1, mode='constant', constant_values=0)

    def at(dy, dx):   # the magnitude at (y + dy, x + dx)
        return mp[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    def first(a):
        return m >= a if mutant == 'first_ge' else m > a

    def second(a):
        return m > a if mutant == 'second_gt' else m >= a

    def diag(a):
        return m >= a if mutant == 'diag_ge' else m > a

    keep_h = first(at(0, -1)) & second(at(0, 1))
    keep_v = first(at(-1, 0)) & second(at(1, 0))
    keep_s = diag(at(-1, -1)) & diag(at(1, 1))
    keep_o = diag(at(-1, 1)) & diag(at(1, -1))
    kept = np.where(horizontal, keep_h,
                    np.where(vertical, keep_v, np.where(same_sign, keep_s, keep_o)))

    cand = kept & (m >= lo if mutant == 'lo_ge' else m > lo)
    strong = cand & (m >= hi if mutant == 'hi_ge' else m > hi)
    if mutant == 'no_hysteresis':
        return cand, strong, strong.copy()
    lab, _ = ndimage.label(cand, structure=FOUR if mutant == 'conn4' else EIGHT)
    edges = cand & np.isin(lab, np.unique(lab[strong]))
    return cand, strong, edges


def canny_ref(bgr, lo, hi, mutant=None):
    """The edge map (bool [h, w]) of one uint8 [h, w, 3] image."""
    return canny_parts(bgr, lo, hi, mutant)[2]


# ---- inputs ------------------------------------------------------------------------
SIZES = ((1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (24, 40), (37, 53))

# (lo, hi): the default, a fractional pair, a swapped pair, lo == hi, a low
# pair, and two pairs for the staircase below: its magnitude-120 pixels are
# candidates at lo = 119.6 (floor 119; rounded or ceiled they are not), and
# are not at lo = 120 (they are with m >= lo)
THRESHOLDS = ((80.0, 200.0), (50.5, 150.25), (200.0, 80.0), (125.0, 125.0), (0.0, 25.0),
              (119.6, 200.0), (120.0, 200.0))


def staircase(h, w):
    """A vertical step edge of height 30 (L1 Sobel magnitude 4 * 30 = 120) in
    the upper half and 60 (240) in the lower: one kept column whose
    magnitudes run 120 ... 120, 180, 240 ... 240 downwards, so at hi = 200
    the magnitude-120 pixels are edges iff they are candidates."""
    img = np.full((h, w, 3), 40, np.uint8)
    img[:h // 2, w // 2:] = 70
    img[h // 2:, w // 2:] = 100
    return img


def noise(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def quantised(rng, h, w):
    """Values 25 k, k < 5: magnitudes are multiples of 25 and tie often."""
    return (25 * rng.integers(0, 5, (h, w, 3))).astype(np.uint8)


def quantised_grey(rng, h, w):
    """The same with the three channels equal: every channel ties."""
    return np.repeat((25 * rng.integers(0, 5, (h, w, 1))).astype(np.uint8), 3, axis=2)


def rectangles(rng, h, w, k=6):
    img = np.empty((h, w, 3), np.uint8)
    img[:] = rng.integers(0, 256, 3)
    for _ in range(k):
        y, x = rng.integers(0, h), rng.integers(0, w)
        img[y:y + rng.integers(1, max(2, h // 2)), x:x + rng.integers(1, max(2, w // 2))] = \
            rng.integers(0, 256, 3)
    return img


def images(h, w):
    """The named fixture images of one size, seeded by the size."""
    rng = np.random.default_rng(1000 * h + w)
    out = []
    for i in range(2):
        out.append(('noise%d' % i, noise(rng, h, w)))
        out.append(('quantised%d' % i, quantised(rng, h, w)))
        out.append(('quantised_grey%d' % i, quantised_grey(rng, h, w)))
        out.append(('rectangles%d' % i, rectangles(rng, h, w)))
    if h >= 8 and w >= 8:
        out.append(('staircase', staircase(h, w)))
    return out


def cases():
    """Every (name, image, lo, hi) the fixture families give."""
    for h, w in SIZES:
        for name, img in images(h, w):
            for lo, hi in THRESHOLDS:
                yield '%dx%d %s %g/%g' % (h, w, name, lo, hi), img, lo, hi


def serpentine(h, w):
    """A corridor 3 px wide of value 70 on ground 40 that runs across the image
    and back in rows 6 px apart (L1 magnitude 4 * 30 = 120: weak at 80 / 200),
    with a 3 x 2 patch of value 160 at its start (magnitude 480: strong).  The
    outline is one chain of weak candidates thousands of pixels long that only
    the patch makes edges: hysteresis has to carry the edge bit all the way."""
    img = np.full((h, w), 40, np.uint8)
    x0, x1 = 4, w - 4
    rows = list(range(4, h - 6, 6))
    for k, y in enumerate(rows):
        img[y:y + 3, x0:x1] = 70
        if k + 1 < len(rows):   # the link to the next run, at alternating ends
            xa = x1 - 3 if k % 2 == 0 else x0
            img[y:y + 9, xa:xa + 3] = 70
    img[rows[0]:rows[0] + 3, x0:x0 + 2] = 160
    return np.repeat(img[..., None], 3, axis=2)


def hysteresis_depth(strong, edges):
    """The number of 8-connected steps from the strong pixels to the edge pixel
    farthest from them, by breadth-first dilation inside the edge set."""
    seen = strong & edges
    depth = 0
    while True:
        grown = ndimage.binary_dilation(seen, structure=EIGHT) & edges
        if np.array_equal(grown, seen):
            return depth
        seen = grown
        depth += 1
