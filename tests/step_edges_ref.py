"""Poses on the step kernels' rare exact paths, for tests/test_step_edges.py and
tests/test_gpu_step_edges.py.

csrc/dtsim_common.h answers floor(v / ts) with the reciprocal and takes the real
division only when the quotient is within 1e-9 of an integer, and answers
sqrt(a) < sqrt(b) on the squares and takes the roots only when they are within
8 eps relative.  Random trajectories reach neither window; the poses built here
sit in both, and a little outside as controls:

  class A  one probe point of _valid_pose (centre, left, right, front) or the
           pose itself (get_lane_pos2's tile) on a tile edge k * ts + d, for
           every edge of the map in x and in z, the outer ones included
  class C  the pose on two edges at once
  class B  poses on the perpendicular bisector of the two curve points that
           level L of bezier_closest compares, ulps of x and z scanned for
           comparisons inside the tie window, of them the ones the squares and
           the roots order differently
  class T  class A poses beside a walker's path with a step counter from which
           the walker arrives at the first, second, third or no Simulator step
           of the decision (the time the exact form of _valid_pose is handed)
  class U  the same for a lane-following bot: the front probe on that edge, in
           the way of a bot driving up its lane
  class P  plain poses mid-road, so that a wave holds both kinds

The arithmetic is the oracle's (oracle/dtsim_ref.py): probe points are the
positions SimulatorRef._valid_pose hands to _drivable_pos, curve points are
bezier_point's, and a bisection path is bezier_closest's.  Only the two
predicates are the kernel's, quoted below.

On the shipped maps (at most 5 tiles wide) the reciprocal form is right at every
edge: the one value within 60 ulps of an edge k <= 16 of a 0.61 grid where the
two floors differ is one ulp below 9 * 0.61.  Hence the 12 x 11 map built here,
whose column 9 and row 9 are not drivable next to drivable 8s.
"""
import math

import numpy as np

from oracle import dtsim_ref as R

TS = R.ROAD_TILE_SIZE
INV_TS = 1.0 / TS
EPS = 2.220446049250313e-16
W, H, BAD = 12, 11, 9
PROBES = ('centre', 'left', 'right', 'front', 'pose')
POSE = 4


# ---- the kernel's predicates (csrc/dtsim_common.h) -------------------------------------
def near_edge(v):
    """floor_div_fast: q = v * inv_ts; r = q - floor(q); near = r < 1e-9 | r > 1 - 1e-9."""
    q = np.asarray(v, np.float64) * INV_TS
    r = q - np.floor(q)
    return (r < 1e-9) | (r > 1.0 - 1e-9)


def floors_differ(v):
    v = np.asarray(v, np.float64)
    return np.floor(v * INV_TS) != np.floor(v / TS)


def near_tie(a, b):
    """bezier_closest_fast: near = !(fabs(b - a) > 8 eps fmax(a, b))."""
    return ~(np.abs(b - a) > 8.0 * EPS * np.maximum(a, b))


def flips(a, b):
    """The squares and the roots order a and b differently."""
    return (a < b) != (np.sqrt(a) < np.sqrt(b))


def dist2(p, x, z):
    """dist2_pt: |p - (x, z)|^2 in the ground plane, unfused (== _norm3's sum, dy = 0)."""
    a, c = p[0] - x, p[2] - z
    return a * a + c * c


# ---- the map ----------------------------------------------------------------------------
_TWO = ('straight/N', 'curve_left/W', 'curve_right/E', 'straight/E', 'curve_left/S',
        'curve_right/N', 'curve_left/N', 'curve_right/W', 'straight/S', 'curve_left/E',
        'curve_right/S')
_MANY = {(2, 2): '4way', (5, 3): '3way_left/S', (3, 6): '3way_right/N', (8, 8): '4way'}


def tiles():
    return [['grass' if BAD in (i, j) else _MANY.get((i, j), _TWO[(i + 3 * j) % len(_TWO)])
             for i in range(W)] for j in range(H)]


DUCKIE = dict(kind='duckie', height=0.08, mesh_min=[-0.5, 0.0, -0.4], mesh_max=[0.5, 1.0, 0.4])
CONE = dict(kind='cone', pos=[10.2, 10.8], height=0.1, mesh_min=[-0.35, 0.0, -0.35],
            mesh_max=[0.35, 1.0, 0.35])
WALKER = dict(DUCKIE, pos=[11.12, 10.8], rotate=90, static=False, wait=0, walk_distance=0.1)
OBJECTS = [CONE, WALKER]       # in the far corner tiles (10..11, 10): only class T is near
# a bot on the lane x = 11.3 of the straight tile (11, 10), driving towards +z (class U)
BOT = dict(kind='duckiebot', height=0.12, mesh_min=[-0.6, 0.0, -0.45], mesh_max=[0.6, 1.0, 0.45],
           static=False, pos=[11.3, 10.3], rotate=-90, velocity=0.1)
BOT_OBJECTS = [CONE, BOT]
BOT_ROWS = 32                  # rows of the bot's path table: t = 0 .. 31


def write_map(path, objects=()):
    import yaml
    doc = {'tiles': tiles()}
    if objects:
        doc['objects'] = [dict(o) for o in objects]
    with open(path, 'w') as f:
        yaml.safe_dump(doc, f)
    return str(path)


# ---- the oracle's probe points ----------------------------------------------------------
class ProbeSim(R.SimulatorRef):
    """SimulatorRef whose _drivable_pos records the point it is asked about:
    probes() returns _valid_pose's centre, left, right and front in its own
    arithmetic."""

    def _drivable_pos(self, pos):
        self.seen.append(np.array(pos, np.float64))
        return True

    def probes(self, x, z, angle):
        self.seen = []
        self._valid_pose(np.array([x, 0.0, z]), angle)
        assert len(self.seen) == 4
        return self.seen


def step_ulps(v, n):
    for _ in range(abs(n)):
        v = math.nextafter(v, math.inf if n > 0 else -math.inf)
    return v


class ShiftedTrig:
    """The oracle's dir / right vectors with cos and sin moved by (dc, ds) ulps:
    what a libm that rounds the other way hands the same arithmetic."""

    def __init__(self, dc, ds):
        self.dc, self.ds = dc, ds

    def __enter__(self):
        self.saved = R.get_dir_vec, R.get_right_vec
        dc, ds = self.dc, self.ds

        def cs(a):
            return step_ulps(math.cos(a), dc), step_ulps(math.sin(a), ds)

        def dir_vec(a):
            c, s = cs(a)
            return np.array([c, 0, -s])

        def right_vec(a):
            c, s = cs(a)
            return np.array([s, 0, c])
        R.get_dir_vec, R.get_right_vec = dir_vec, right_vec

    def __exit__(self, *exc):
        R.get_dir_vec, R.get_right_vec = self.saved


def _grid(ps):
    return [(math.floor(p[0] / TS), math.floor(p[2] / TS)) for p in ps]


def libm_proof(pr, x, z, angle, axis, probe, v):
    """The device's sincos may differ from libm's in the last place.  True when
    that changes nothing here: with cos and sin each an ulp either way every
    probe stays in its tile, and the probe under test stays inside (or outside)
    the window and a value on which the two floors differ (or agree).  (Angle
    0.0 has cos 1 and sin 0 everywhere.)"""
    if angle == 0.0:
        return True
    base = _grid(pr.probes(x, z, angle))
    label = (bool(near_edge(v)), bool(floors_differ(v)))
    for dc in (-1, 0, 1):
        for ds in (-1, 0, 1):
            if dc == 0 and ds == 0:
                continue
            with ShiftedTrig(dc, ds):
                ps = pr.probes(x, z, angle)
            if _grid(ps) != base:
                return False
            if probe != POSE:
                pv = ps[probe][2 * axis]
                if (bool(near_edge(pv)), bool(floors_differ(pv))) != label:
                    return False
    return True


def place(pr, axis, probe, target, other, angle):
    """The pose coordinate on `axis` that puts `probe` on `target` (exactly where
    float64 allows, else as near as it gets), and the value the probe then has."""
    if probe == POSE:
        return target, target

    def val(c):
        ps = pr.probes(c, other, angle) if axis == 0 else pr.probes(other, c, angle)
        return float(ps[probe][2 * axis])
    c = target
    for _ in range(4):
        v = val(c)
        if v == target:
            return c, v
        c = c - (v - target)
    _, c = min((abs(val(cc) - target), cc) for cc in (step_ulps(c, n) for n in range(-3, 4)))
    return c, val(c)


# ---- class A ------------------------------------------------------------------------------
ULPS = (-3, -2, -1, 0, 1, 2, 3)
INSIDE = (-5e-10, 5e-10)        # inside the 1e-9 window of the quotient
OUTSIDE = (-2e-9, 2e-9)         # controls: outside it
# the angle that makes a probe the furthest point along +x / +z, so that the pose is valid
# right up to the edge: x: front at 0.0, right at 1.3, left at -1.7; z: right at 0.0,
# front at -1.7, left at 2.9
SECOND_ANGLE = ((2.9, -1.7, 1.3, 2.9, 1.3), (1.3, 2.9, 1.3, -1.7, 2.9))


def edge_targets(k):
    e = k * TS
    out = [(step_ulps(e, n), False) for n in ULPS]
    out += [(e + d, False) for d in INSIDE]
    out += [(e + d, True) for d in OUTSIDE]
    return out


def class_a(pr):
    rows = []
    for axis in (0, 1):
        for k in range((W if axis == 0 else H) + 1):
            for probe in range(5):
                other = ((2 * k + probe) % BAD + 0.37) * TS
                for angle0 in (0.0, SECOND_ANGLE[axis][probe]):
                    for target, control in edge_targets(k):
                        if angle0 and abs(target) < 1e-300:
                            continue    # a sum that cancels to 0 +- ulps: angle 0.0 only
                        for attempt in range(8):
                            angle = angle0 + attempt * 2.0 ** -12 if angle0 else 0.0
                            c, v = place(pr, axis, probe, target, other, angle)
                            x, z = (c, other) if axis == 0 else (other, c)
                            if libm_proof(pr, x, z, angle, axis, probe, v):
                                break
                        else:
                            raise AssertionError(('no libm-proof pose', axis, k, probe, target))
                        rows.append(dict(cls='A', x=x, z=z, angle=angle, axis=axis, k=k,
                                         probe=probe, v=v, control=control))
    return rows


def class_c():
    rows = []
    for (kx, kz) in ((0, 0), (BAD, BAD), (W, H), (5, BAD), (BAD, 4)):
        for nx in (-1, 0, 1):
            for nz in (-1, 0, 1):
                rows.append(dict(cls='C', x=step_ulps(kx * TS, nx), z=step_ulps(kz * TS, nz),
                                 angle=0.0, axis=2, k=kx, probe=POSE, v=step_ulps(kx * TS, nx)))
    return rows


# ---- class B ------------------------------------------------------------------------------
def curve_angle(curves, ci):
    """A heading for which closest_curve_point picks curve ci: 0.2 rad off the curve's own
    (not along it: acos next to 1 would magnify the last place of the device's sincos)."""
    h = curves[ci, -1, :] - curves[ci, 0, :]
    angle = math.atan2(-h[2], h[0]) + 0.2
    dots = R.tile_headings(curves) @ R.get_dir_vec(angle)
    assert int(np.argmax(dots)) == ci
    return angle


def scan_level(tile, ci, level, m, n_u=121, n_ulp=40, keep=(8, 16, 2)):
    """Candidates around the bisector of B(tb) and B(tt), the points level `level`
    compares on interval m, kept when bezier_closest's earlier levels lead there:
    up to keep[0] flips, keep[1] other in-window ones, keep[2] controls."""
    curves, (i, j) = tile['curves'], tile['coords']
    cps = curves[ci]
    tb, tt = m / 2.0 ** (level - 1), (m + 1) / 2.0 ** (level - 1)
    pb, pt = R.bezier_point(cps, tb), R.bezier_point(cps, tt)
    d = pt - pb
    nrm = np.array([-d[2], d[0]]) / math.hypot(d[0], d[2])
    u = np.linspace(-0.3 * TS, 0.3 * TS, n_u)
    bx, bz = 0.5 * (pb[0] + pt[0]) + u * nrm[0], 0.5 * (pb[2] + pt[2]) + u * nrm[1]
    n = np.arange(-n_ulp, n_ulp + 1, dtype=np.float64)
    x = np.concatenate([(bx[:, None] + n[None, :] * np.spacing(bx)[:, None]).ravel(),
                        np.repeat(bx, len(n))])
    z = np.concatenate([np.repeat(bz, len(n)),
                        (bz[:, None] + n[None, :] * np.spacing(bz)[:, None]).ravel()])
    inside = (np.floor(x / TS) == i) & (np.floor(z / TS) == j) & ~near_edge(x) & ~near_edge(z)
    x, z = x[inside], z[inside]
    a, b = dist2(pb, x, z), dist2(pt, x, z)
    win, flip = near_tie(a, b), flips(a, b)
    assert not (flip & ~win).any()      # the window covers every flip
    angle = curve_angle(curves, ci)
    rows = []
    for sel, cap in ((flip, keep[0]), (win & ~flip, keep[1]), (~win, keep[2])):
        idx = np.flatnonzero(sel)
        if len(idx) > 4 * cap:
            idx = idx[np.linspace(0, len(idx) - 1, 4 * cap).astype(int)]
        got = 0
        for q in idx:
            if got == cap:
                break
            p = np.array([x[q], 0.0, z[q]])
            if R.bezier_closest(cps, p, n=level - 1) != 0.5 * (tb + tt):
                continue
            got += 1
            rows.append(dict(cls='B', x=float(x[q]), z=float(z[q]), angle=angle, level=level,
                             in_window=bool(win[q]), flip=bool(flip[q]),
                             control=not bool(win[q])))
    return rows


def class_b(mp):
    rows = []
    picks = []
    for kind in ('curve_left', 'curve_right', 'straight'):
        picks.append(next(t for t in mp.drivable_tiles if t['kind'] == kind
                          and 1 <= t['coords'][0] <= 7 and 1 <= t['coords'][1] <= 7))
    for tile in picks:
        for level in (1, 2, 3):
            for ci in (0, 1):
                for m in range(2 ** (level - 1)):
                    rows += scan_level(tile, ci, level, m)
        for level in (4, 5, 6, 7, 8):       # the same budget a level; whatever turns up
            last = 2 ** (level - 1) - 1
            for m in (0, last // 2, last):
                rows += scan_level(tile, 0, level, m, n_u=41, keep=(4, 4, 1))
    return rows


# ---- class T ------------------------------------------------------------------------------
def class_t(pr):
    """The centre probe on the edge x = 11 ts, 0.2 m down the walker's path: the
    walker reaches the agent's box at index `hit`, so a decision that starts at
    step count hit - 1 - r0 ends at its Simulator step r0 + 1 (r0 = 3: not yet)."""
    import walkers_ref as WR
    sim = WR.WalkerSimRef(tiles(), objects=OBJECTS)
    w = sim.walkers[0]
    z = w.pos[2] - 0.2
    rows = []
    for target, control in ((11 * TS, False), (step_ulps(11 * TS, 1), False),
                            (11 * TS + 5e-10, False), (11 * TS + 2e-9, True)):
        x, v = place(pr, 0, 0, target, z, 0.0)
        pos = np.array([x, 0.0, z])
        hit = None
        for idx in range(w.K + 1):
            sim.place(idx)
            if not sim._valid_pose(pos, 0.0):
                hit = idx
                break
        assert hit is not None and hit >= 5, hit
        for r0 in range(4):
            rows.append(dict(cls='T', x=x, z=z, angle=0.0, axis=0, k=11, probe=0, v=v,
                             control=control, step_count=hit - 1 - r0, r0=r0))
    return rows


def bot_sim():
    import bots_ref as BR
    path = BR.own_path(tiles(), BOT_OBJECTS, BOT_ROWS)
    return BR.BotSimRef(tiles(), path, objects=BOT_OBJECTS), path


def class_u(pr):
    """Facing -x (angle pi: cos -1) with the front probe on the edge x = 11 ts,
    the box reaches over the bot's lane 0.25 m ahead of its home: the bot
    drives into it at row `hit` of its path, and the step counters are class
    T's."""
    sim, _ = bot_sim()
    z = sim.bots[0].pos[2] + 0.25
    rows = []
    for target, control in ((11 * TS, False), (step_ulps(11 * TS, 1), False),
                            (11 * TS + 5e-10, False), (11 * TS + 2e-9, True)):
        x, v = place(pr, 0, 3, target, z, math.pi)
        assert libm_proof(pr, x, z, math.pi, 0, 3, v)
        pos = np.array([x, 0.0, z])
        hit = None
        for idx in range(BOT_ROWS):
            sim.place(idx)
            if not sim._valid_pose(pos, math.pi):
                hit = idx
                break
        assert hit is not None and 5 <= hit < BOT_ROWS - 3, hit
        for r0 in range(4):
            rows.append(dict(cls='U', x=x, z=z, angle=math.pi, axis=0, k=11, probe=3, v=v,
                             control=control, step_count=hit - 1 - r0, r0=r0))
    return rows


def class_p(n=384):
    rng = np.random.default_rng(5)
    return [dict(cls='P', x=(rng.integers(1, 8) + rng.uniform(0.2, 0.8)) * TS,
                 z=(rng.integers(1, 8) + rng.uniform(0.2, 0.8)) * TS,
                 angle=rng.uniform(-math.pi, math.pi), control=True) for _ in range(n)]


# ---- the batch ----------------------------------------------------------------------------
class ReciprocalSim(R.SimulatorRef):
    """SimulatorRef with the reciprocal form of get_grid_coords alone: what a
    kernel that never took the division would compute."""

    def get_grid_coords(self, abs_pos):
        x, _, z = abs_pos
        return int(math.floor(x * INV_TS)), int(math.floor(z * INV_TS))


class Cases:
    """The batch: x, z, angle, step_count and a label per env, in a fixed
    shuffled order (so a fan-kernel wave of 16 envs mixes flagged and plain
    quads), padded with plain poses to a multiple of 16."""

    FIELDS = dict(cls='U1', x='f8', z='f8', angle='f8', axis='i4', k='i4', probe='i4', v='f8',
                  control='?', level='i4', r0='i4', in_window='?', flip='?', step_count='u4')

    def __init__(self):
        self.rows = tiles()
        self.map = R.MapRef(self.rows)
        pr = ProbeSim(self.rows)
        rows = (class_a(pr) + class_c() + class_b(self.map) + class_t(pr) + class_u(pr) +
                class_p())
        rows += class_p(384 + -len(rows) % 16)[384:]
        order = np.random.default_rng(17).permutation(len(rows))
        self.n = len(rows)
        for name, dt in self.FIELDS.items():
            default = np.nan if dt == 'f8' else ('' if dt == 'U1' else 0)
            setattr(self, name, np.array([rows[q].get(name, default) for q in order], dtype=dt))
        # the quotient under test: of class A / T / U the probe's value, of class C both
        edge = np.isin(self.cls, ('A', 'T', 'U'))
        self.in_window[edge] = near_edge(self.v[edge])
        c = self.cls == 'C'
        self.in_window[c] = near_edge(self.x[c]) | near_edge(self.z[c])
        self.differ = np.zeros(self.n, bool)
        self.differ[edge] = floors_differ(self.v[edge])
        self.differ[c] = floors_differ(self.x[c]) | floors_differ(self.z[c])
        # any flag at all, by the kernel's predicates on the oracle's probe points (class B
        # has its own from the scan): which quads take a fallback
        self.near = self.in_window.copy()
        for q in range(self.n):
            if self.cls[q] != 'B':
                ps = pr.probes(self.x[q], self.z[q], self.angle[q])
                vals = [p[0] for p in ps] + [p[2] for p in ps] + [self.x[q], self.z[q]]
                self.near[q] |= bool(near_edge(vals).any())
        # where the two floors differ: both answers, from the oracle and from its
        # reciprocal-only twin
        exact, recip = R.SimulatorRef(self.rows), ReciprocalSim(self.rows)
        self.div_valid = np.ones(self.n, bool)
        self.rcp_valid = np.ones(self.n, bool)
        self.div_tile = np.full(self.n, -2, np.int32)
        self.rcp_tile = np.full(self.n, -2, np.int32)
        for q in np.flatnonzero(self.differ):
            pos = np.array([self.x[q], 0.0, self.z[q]])
            for sim, valid, tile in ((exact, self.div_valid, self.div_tile),
                                     (recip, self.rcp_valid, self.rcp_tile)):
                valid[q] = sim._valid_pose(pos, self.angle[q])
                sim.cur_pos = pos
                tile[q] = R.EnvironmentWrapperRef(sim).tile_index()

    def subset(self, want):
        """Indices of a batch of len(want) rounded up to 16 with plain poses."""
        idx = list(np.flatnonzero(want))
        plain = [q for q in np.flatnonzero(self.cls == 'P') if not want[q]]
        idx += plain[:-len(idx) % 16]
        assert len(idx) % 16 == 0
        return np.array(sorted(idx))


_CASES = None


def cases():
    """Built once a process, never changed."""
    global _CASES
    if _CASES is None:
        _CASES = Cases()
    return _CASES
