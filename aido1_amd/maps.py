"""Tile maps -> the C ABI's ``dt_map`` arrays.

Follows upstream Simulator._load_map / _get_curve (un-vendored gym-duckietown,
aido1 era): tiles "kind/orient" are drivable with
orient index ['S','E','N','W'], anything else without a slash is an off-road
tile, a tile containing "4" is a 4-way intersection (angle 2), anything else
without a slash is an off-road tile, 'empty' is no tile at all.  Each drivable
tile gets its cubic Bezier lane curves -- 2 for straight / curves, 6 for a
3-way, 12 for a 4-way (its 3-curve template at all four rotations) -- the
unit-tile template scaled by the tile size, rotated by ``pts @ R_y(angle *
pi / 2)`` (quaternion-form matrix) and translated to the tile centre.  The
computation is done once per map on the host in float64 with the same numpy
expressions, so the control points are the reference's.

Curves are stored compactly for the C ABI (dt_map): tile t owns curves
curve_start[t] .. curve_start[t+1]-1 of ``curves`` [C,4,3] / ``headings`` [C,3].

Static objects follow upstream Simulator._load_objects and
collision.py: world position = tile_size * (x, y, z), scale = height /
mesh max y, footprint corners = the mesh's x/z box scaled, offset to the
position and rotated about it by `rotate` degrees (rotate_point), axes =
generate_norm (eigenvectors of the corners' covariance -- for a square
footprint that is the world x/z axes whatever the rotation, as upstream),
safety radius = SAFETY_RAD_MULT * hypot(max |x|, max |z|) * scale.  An object
is collidable (checked by _collision / proximity_penalty2) when it is static,
not a traffic light, and its box meets a drivable tile (_collidable_object);
every object counts for _inconvenient_spawn.  The meshes are not in this
container, so the per-kind boxes below are assumptions (override them per
object with ``mesh_min`` / ``mesh_max``).

Walkers (upstream DuckieObj, recalled; parity unpinned like the static objects):
a ``duckie`` with ``static: false`` waits `wait` seconds, walks `vel` metres a
Simulator step along its heading until it is past `walk_distance` + 0.25,
turns round, waits, walks back, and so on.  Without domain randomisation that
is a function of time alone, so here a walker's displacement is a closed form
of the env's Simulator step counter (walker_index; include/dtsim.h
dt_set_walkers restates it) and the walker is at home whenever the counter is
0 -- upstream keeps its objects moving across resets; build-defined.  A walker
is always collidable.

Lane-following bots (upstream DuckiebotObj of the AIDO1 era, recalled; parity
unpinned): a ``duckiebot`` with ``static: false`` drives along the lane centre
by pure pursuit.  It reads nothing of the agent, so its pose after t Simulator
steps from home is a function of t alone -- a table the device computes once
(dt_bot_path, include/dtsim.h) and the step and render kernels index with the
env's step counter.  Opt-in: ``load_map(..., lane_bots=True)``; without the
switch such an entry is refused, as is any other kind with ``static: false``.
"""
import math
import os
from dataclasses import dataclass

import numpy as np
import yaml

MAP_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'maps')

# the agent's box, which a moving bot takes (dt_config.robot_width / robot_length)
ROBOT_WIDTH = 0.13 + 0.02
ROBOT_LENGTH = 0.18
SAFETY_RAD_MULT = 1.8
MIN_SPAWN_OBJ_DIST = 0.25
DEFAULT_FRAMERATE = 30
# upstream DuckieObj defaults: metres per Simulator step (not scaled by
# delta_time), seconds, and the margin added to walk_distance
WALKER_VEL = 0.02
WALKER_WAIT = 8.0
WALKER_EXTRA_DIST = 0.25
# upstream DuckiebotObj defaults: metres a second, metres; then the constants of
# its wheel controller (gain, trim, wheel radius, motor constant k, limit)
BOT_VELOCITY = 0.1
BOT_FOLLOW_DIST = 0.3
BOT_GAIN, BOT_TRIM, BOT_RADIUS, BOT_K, BOT_LIMIT = 2.0, 0.0, 0.0318, 27.0, 1.0
BOT_STRIDE = 7       # DT_BOT_STRIDE: velocity, follow_dist, gain, trim, radius, k, limit
MAX_BOT_ROWS = 131072            # DT_MAX_BOT_ROWS
MAX_BOT_BYTES = 256 << 20        # of the [rows, n, 20] float64 table
# mesh bounding boxes (min, max) in mesh units, y up -- ASSUMED (the upstream
# .obj meshes are absent); with `height` only their proportions matter
MESH_EXTENTS = {
    'duckie': ((-0.5, 0.0, -0.4), (0.5, 1.0, 0.4)),
    'cone': ((-0.35, 0.0, -0.35), (0.35, 1.0, 0.35)),
    'barrier': ((-1.0, 0.0, -0.2), (1.0, 1.0, 0.2)),
    'duckiebot': ((-0.6, 0.0, -0.45), (0.6, 1.0, 0.45)),
    'truck': ((-1.2, 0.0, -0.5), (1.2, 1.0, 0.5)),
    'bus': ((-1.5, 0.0, -0.5), (1.5, 1.0, 0.5)),
    'house': ((-0.6, 0.0, -0.5), (0.6, 1.0, 0.5)),
    'building': ((-0.6, 0.0, -0.6), (0.6, 1.0, 0.6)),
    'tree': ((-0.4, 0.0, -0.4), (0.4, 1.0, 0.4)),
    'trafficlight': ((-0.1, 0.0, -0.1), (0.1, 1.0, 0.1)),
    'sign': ((-0.15, 0.0, -0.02), (0.15, 1.0, 0.02)),
}

TILE_EMPTY, TILE_OFFROAD, TILE_STRAIGHT, TILE_CURVE_LEFT, TILE_CURVE_RIGHT = -1, 0, 1, 2, 3
TILE_3WAY_LEFT, TILE_3WAY_RIGHT, TILE_4WAY = 4, 5, 6
KIND_CODES = {'straight': TILE_STRAIGHT, 'curve_left': TILE_CURVE_LEFT,
              'curve_right': TILE_CURVE_RIGHT, '3way_left': TILE_3WAY_LEFT,
              '3way_right': TILE_3WAY_RIGHT, '4way': TILE_4WAY}

# unit-tile lane templates (two lanes per tile, right-hand traffic)
LANE_TEMPLATES = {
    TILE_STRAIGHT: np.array([
        [[-0.20, 0, -0.50], [-0.20, 0, -0.25], [-0.20, 0, 0.25], [-0.20, 0, 0.50]],
        [[0.20, 0, 0.50], [0.20, 0, 0.25], [0.20, 0, -0.25], [0.20, 0, -0.50]],
    ]),
    TILE_CURVE_LEFT: np.array([
        [[-0.20, 0, -0.50], [-0.20, 0, 0.00], [0.00, 0, 0.20], [0.50, 0, 0.20]],
        [[0.50, 0, -0.20], [0.30, 0, -0.20], [0.20, 0, -0.30], [0.20, 0, -0.50]],
    ]),
    TILE_CURVE_RIGHT: np.array([
        [[-0.20, 0, -0.50], [-0.20, 0, -0.20], [-0.30, 0, -0.20], [-0.50, 0, -0.20]],
        [[-0.50, 0, 0.20], [-0.30, 0, 0.20], [0.30, 0, 0.00], [0.20, 0, -0.50]],
    ]),
    # 3-way: straight through both ways + the four turns to / from the side road
    TILE_3WAY_LEFT: np.array([
        [[-0.20, 0, -0.50], [-0.20, 0, -0.25], [-0.20, 0, 0.25], [-0.20, 0, 0.50]],
        [[-0.20, 0, -0.50], [-0.20, 0, 0.00], [0.00, 0, 0.20], [0.50, 0, 0.20]],
        [[0.20, 0, 0.50], [0.20, 0, 0.25], [0.20, 0, -0.25], [0.20, 0, -0.50]],
        [[0.50, 0, -0.20], [0.30, 0, -0.20], [0.20, 0, -0.20], [0.20, 0, -0.50]],
        [[0.20, 0, 0.50], [0.20, 0, 0.20], [0.30, 0, 0.20], [0.50, 0, 0.20]],
        [[0.50, 0, -0.20], [0.30, 0, -0.20], [-0.20, 0, 0.00], [-0.20, 0, 0.50]],
    ]),
    # 4-way: left / straight / right from one entry, rotated to all four sides
    TILE_4WAY: np.array([
        [[-0.20, 0, -0.50], [-0.20, 0, 0.00], [0.00, 0, 0.20], [0.50, 0, 0.20]],
        [[-0.20, 0, -0.50], [-0.20, 0, -0.25], [-0.20, 0, 0.25], [-0.20, 0, 0.50]],
        [[-0.20, 0, -0.50], [-0.20, 0, -0.20], [-0.30, 0, -0.20], [-0.50, 0, -0.20]],
    ]),
}
LANE_TEMPLATES[TILE_3WAY_RIGHT] = LANE_TEMPLATES[TILE_3WAY_LEFT]  # upstream: kind.startswith('3way')


def rotation_y(angle):
    """Counter-clockwise rotation about +y, upstream gen_rot_matrix form."""
    axis = np.array([0, 1, 0])
    axis = axis / math.sqrt(np.dot(axis, axis))
    a = math.cos(angle / 2.0)
    b, c, d = -axis * math.sin(angle / 2.0)
    return np.array([
        [a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
        [2 * (b * c + a * d), a * a + c * c - b * b - d * d, 2 * (c * d - a * b)],
        [2 * (b * d - a * c), 2 * (c * d + a * b), a * a + d * d - b * b - c * c],
    ])


# ---- static objects: upstream collision.py restated -----------------------------------
def rotate_point(px, py, cx, cy, theta):
    """Rotate (px, py) about (cx, cy) by theta (upstream graphics/collision)."""
    dx = px - cx
    dy = py - cy
    new_dx = dx * math.cos(theta) + dy * math.sin(theta)
    new_dy = dy * math.cos(theta) - dx * math.sin(theta)
    return cx + new_dx, cy + new_dy


def generate_corners(pos, min_coords, max_coords, theta, scale):
    """Footprint corners [4, 2] (x, z) of an object at world `pos`."""
    px, pz = pos[0], pos[-1]
    return np.array([
        rotate_point(min_coords[0] * scale + px, min_coords[-1] * scale + pz, px, pz, theta),
        rotate_point(max_coords[0] * scale + px, min_coords[-1] * scale + pz, px, pz, theta),
        rotate_point(max_coords[0] * scale + px, max_coords[-1] * scale + pz, px, pz, theta),
        rotate_point(min_coords[0] * scale + px, max_coords[-1] * scale + pz, px, pz, theta),
    ])


def generate_norm(corners):
    """The box's two axes (rows, unit): eigenvectors of the corners' covariance."""
    ca = np.cov(corners, y=None, rowvar=False, bias=True)
    _, vect = np.linalg.eig(ca)
    return np.ascontiguousarray(vect.T.real)


def _proj(corners, axis):
    p = corners @ axis
    return p.min(), p.max()


def sat_intersects(c1, n1, c2, n2):
    """Separating-axis test of two boxes (corners [4,2], axes [2,2]): no axis of
    either separates their closed projection intervals."""
    for axis in np.concatenate([n1, n2]):
        a0, a1 = _proj(c1, axis)
        b0, b1 = _proj(c2, axis)
        if a1 < b0 or b1 < a0:
            return False
    return True


def tile_corners(i, j, width):
    px, pz = i * width, j * width
    return np.array([[px, pz], [px + width, pz], [px + width, pz + width], [px, pz + width]])


def find_candidate_tiles(corners, tile_size):
    mn = np.floor(np.amin(corners, axis=0) / tile_size).astype(int)
    mx = np.floor(np.amax(corners, axis=0) / tile_size).astype(int)
    return [(x, y) for x in range(mn[0], mx[0] + 1) for y in range(mn[1], mx[1] + 1)]


def agent_boundbox(true_pos, width, length, f_vec, r_vec):
    """Upstream agent_boundbox: the [4, 2] (x, z) corners of a width x length
    box about true_pos (x, y, z) with forward / right vectors f_vec / r_vec."""
    hwidth = width / 2
    hlength = length / 2
    return np.array([
        true_pos - hwidth * r_vec - hlength * f_vec,
        true_pos + hwidth * r_vec - hlength * f_vec,
        true_pos + hwidth * r_vec + hlength * f_vec,
        true_pos - hwidth * r_vec + hlength * f_vec,
    ])[:, [0, 2]]


def bot_rows(max_steps, frame_skip, max_env_steps):
    """Rows of a bot path table that a wrapped run never leaves: the largest
    Simulator step counter an episode reaches, plus row 0.  EnvironmentWrapper
    counts Simulator.step calls (frame_skip updates each) and ends the episode
    once the count exceeds max_env_steps; the Simulator ends it at the first
    whole Simulator.step that reaches max_steps (so at max_steps rounded up to
    a multiple of frame_skip)."""
    fs = int(frame_skip)
    by_sim = -(-int(max_steps) // fs) * fs
    return min(by_sim, fs * (int(max_env_steps) + 1)) + 1


def walker_index(t, W, K):
    """Steps of `vel` a walker stands from home at Simulator step count t: it
    waits W steps, walks K, waits W, walks K back, ... (period 2 (W + K)).
    All integer."""
    P = W + K
    leg, p = divmod(int(t), P)
    m = max(0, p - W)
    return m if leg % 2 == 0 else K - m


@dataclass
class MapObject:
    kind: str
    pos: np.ndarray            # world (x, y, z)
    rotate: float              # degrees
    scale: float
    min_coords: np.ndarray
    max_coords: np.ndarray
    static: bool
    corners: np.ndarray        # [4, 2]
    norms: np.ndarray          # [2, 2]
    safety_radius: float
    collidable: bool = False
    # a walker (kind duckie, static false): metres per Simulator step, seconds,
    # metres; W wait steps and K walk steps a leg (walker_index); 0 when static
    vel: float = 0.0
    wait: float = 0.0
    walk_distance: float = 0.0
    W: int = 0
    K: int = 0
    # a lane-following bot (kind duckiebot, static false): metres a second, metres
    velocity: float = 0.0
    follow_dist: float = 0.0

    @property
    def bot(self):
        return not self.static and self.kind == 'duckiebot'

    @property
    def walker(self):
        return not self.static and not self.bot

    @property
    def bot_params(self):
        """The DT_BOT_STRIDE doubles of dt_bot_path for this bot."""
        return [self.velocity, self.follow_dist, BOT_GAIN, BOT_TRIM, BOT_RADIUS, BOT_K,
                BOT_LIMIT]

    @property
    def heading(self):
        """(hx, hz) = get_dir_vec(radians(rotate))."""
        a = math.radians(self.rotate)
        return math.cos(a), -math.sin(a)

    @property
    def spawn_radius(self):
        """_inconvenient_spawn: max(max_coords) * 0.5 * scale + MIN_SPAWN_OBJ_DIST."""
        return float(np.max(self.max_coords)) * 0.5 * self.scale + MIN_SPAWN_OBJ_DIST

    def record(self):
        """The DT_OBJ_STRIDE doubles of include/dtsim.h for this object."""
        r = np.zeros(20, np.float64)
        r[0:3] = self.pos
        r[3] = self.safety_radius
        r[4:12] = self.corners.reshape(-1)
        r[12:16] = self.norms.reshape(-1)
        for a in range(2):
            r[16 + 2 * a:18 + 2 * a] = _proj(self.corners, self.norms[a])
        return r


def _parse_geometry(desc, tile_size):
    """The MapObject of a map entry at its (home) pose."""
    kind = desc['kind']
    pos = desc['pos']
    x, z = pos[0:2]
    y = pos[2] if len(pos) == 3 else 0.0
    world = tile_size * np.array((x, y, z), np.float64)
    if 'mesh_min' in desc or 'mesh_max' in desc:
        mn, mx = desc['mesh_min'], desc['mesh_max']
    elif kind in MESH_EXTENTS or kind.startswith('sign'):
        mn, mx = MESH_EXTENTS[kind if kind in MESH_EXTENTS else 'sign']
    else:
        raise ValueError('object kind %r has no known extents: give mesh_min / mesh_max' % kind)
    mn = np.array(mn, np.float64)
    mx = np.array(mx, np.float64)
    if 'height' in desc and 'scale' in desc:
        raise ValueError('cannot specify both height and scale')
    scale = desc['height'] / mx[1] if 'height' in desc else float(desc.get('scale', 1.0))
    static = bool(desc.get('static', True))
    rotate = float(desc.get('rotate', 0.0))
    corners = generate_corners(world, mn, mx, np.radians(rotate), scale)
    ext = np.max([np.abs(mn), np.abs(mx)], axis=0)
    safety = SAFETY_RAD_MULT * (np.hypot(ext[0], ext[2]) * scale)
    return MapObject(kind, world, rotate, scale, mn, mx, static, corners,
                     generate_norm(corners), float(safety))


def parse_object(desc, tile_size):
    """A static object.  (A map's dynamic entries go through parse_walker.)"""
    if not bool(desc.get('static', True)):
        raise NotImplementedError('dynamic (non-static) objects are not supported')
    return _parse_geometry(desc, tile_size)


def parse_walker(desc, tile_size, frame_rate=DEFAULT_FRAMERATE):
    """A walker: `kind: duckie` with `static: false`.  Any other dynamic kind
    is refused (the lane-following duckiebot is parse_bot's, behind
    `lane_bots=True`)."""
    if bool(desc.get('static', True)) or desc['kind'] != 'duckie':
        raise NotImplementedError(
            'dynamic (non-static) objects of kind %r are not supported (only the walking '
            'duckie is, and with lane_bots=True the lane-following duckiebot)' % desc['kind'])
    obj = _parse_geometry(desc, tile_size)
    obj.vel = float(desc.get('vel', WALKER_VEL))
    obj.wait = float(desc.get('wait', WALKER_WAIT))
    obj.walk_distance = float(desc.get('walk_distance', tile_size))
    if not (obj.vel > 0.0 and math.isfinite(obj.vel)) or obj.wait < 0.0 or \
            not math.isfinite(obj.wait) or not math.isfinite(obj.walk_distance):
        raise ValueError('walker needs vel > 0, wait >= 0 and a finite walk_distance')
    obj.W = int(round(obj.wait * frame_rate))
    D = obj.walk_distance + WALKER_EXTRA_DIST
    k = max(1, int(D / obj.vel) - 2) if D > 0.0 else 1
    while not float(k) * obj.vel > D:   # the smallest k >= 1 with float64(k) * vel > D
        k += 1
    while k > 1 and float(k - 1) * obj.vel > D:
        k -= 1
    obj.K = k
    if obj.W >= 1 << 24 or obj.K >= 1 << 24:
        raise ValueError('walker wait / walk steps must stay below 2^24')
    obj.collidable = True
    return obj


def parse_bot(desc, tile_size):
    """A lane-following bot: `kind: duckiebot` with `static: false` (what
    `lane_bots=True` sends here).  Its home is the entry's pose; its record at
    home is the static object's."""
    if bool(desc.get('static', True)) or desc['kind'] != 'duckiebot':
        raise NotImplementedError('parse_bot takes a duckiebot with static: false, not %r'
                                  % desc['kind'])
    obj = _parse_geometry(desc, tile_size)
    obj.velocity = float(desc.get('velocity', BOT_VELOCITY))
    obj.follow_dist = float(desc.get('follow_dist', BOT_FOLLOW_DIST))
    if not (obj.velocity >= 0.0 and math.isfinite(obj.velocity)) or \
            not (obj.follow_dist > 0.0 and math.isfinite(obj.follow_dist)):
        raise ValueError('bot needs a finite velocity >= 0 and a finite follow_dist > 0')
    obj.collidable = True
    return obj


@dataclass
class TileMap:
    name: str
    width: int
    height: int
    tile_size: float
    kind: np.ndarray         # [H*W] int8
    orient: np.ndarray       # [H*W] int8
    curves: np.ndarray       # [C, 4, 3] float64, tile t's at curve_start[t]:curve_start[t+1]
    headings: np.ndarray     # [C, 3] float64
    curve_start: np.ndarray  # [H*W + 1] int32
    rows: list
    objects: list = None     # [MapObject]

    def tile_curves(self, t):
        return self.curves[self.curve_start[t]:self.curve_start[t + 1]]

    @property
    def object_table(self):
        """[K, 20] float64 records of the collidable objects (dt_map.objects):
        the static ones in load order, then the walkers, then the bots (both at
        home), each in load order."""
        recs = [o.record() for o in self._collidables()]
        return np.array(recs, np.float64).reshape(-1, 20)

    def _collidables(self):
        objs = [o for o in (self.objects or []) if o.collidable]
        return [o for o in objs if o.static] + [o for o in objs if o.walker] + \
            [o for o in objs if o.bot]

    @property
    def has_walkers(self):
        return any(o.walker for o in (self.objects or []))

    @property
    def bots(self):
        """The bots in load order (the order of every bot table's columns)."""
        return [o for o in (self.objects or []) if o.bot]

    @property
    def bot_home(self):
        """[n, 3] float64 (x, z, angle) of the bots at home (dt_bot_path)."""
        return np.array([[o.pos[0], o.pos[2], math.radians(o.rotate)] for o in self.bots],
                        np.float64).reshape(-1, 3)

    @property
    def bot_param_table(self):
        """[n, BOT_STRIDE] float64 (dt_bot_path)."""
        return np.array([o.bot_params for o in self.bots], np.float64).reshape(-1, BOT_STRIDE)

    @property
    def bot_object_rows(self):
        """[n] int32: each bot's row of object_table (dt_set_bots)."""
        c = self._collidables()
        return np.array([next(i for i, x in enumerate(c) if x is o) for o in self.bots], np.int32)

    @property
    def bot_render_rows(self):
        """[n] int32: each bot's row of render_table (dt_render_bots)."""
        objs = self.objects or []
        return np.array([next(i for i, x in enumerate(objs) if x is o) for o in self.bots],
                        np.int32)

    def _bot_corners(self, path, robot_width=ROBOT_WIDTH, robot_length=ROBOT_LENGTH):
        """[rows, n, 4, 2]: row 0 the bots' static corners, rows >= 1 the
        agent_boundbox of the pose path[t, b] = (x, z, angle)."""
        path = np.asarray(path, np.float64)
        rows, n = path.shape[0], len(self.bots)
        assert path.shape == (rows, n, 3), path.shape
        out = np.zeros((rows, n, 4, 2), np.float64)
        for b, o in enumerate(self.bots):
            out[0, b] = o.corners
            for t in range(1, rows):
                x, z, a = path[t, b]
                f = np.array([math.cos(a), 0.0, -math.sin(a)])
                r = np.array([math.sin(a), 0.0, math.cos(a)])
                out[t, b] = agent_boundbox(np.array([x, o.pos[1], z]), robot_width, robot_length,
                                           f, r)
        return out

    def bot_records(self, path, robot_width=ROBOT_WIDTH, robot_length=ROBOT_LENGTH):
        """[rows, n, 20] float64 (dt_set_bots): row 0 is record(); row t >= 1
        holds the box upstream's DuckiebotObj._update_pos makes at path[t]:
        corners = agent_boundbox(pos_t, robot_width, robot_length, dir, right),
        axes = generate_norm of them, their projections, centre = pos_t; the
        safety radius does not change."""
        cor = self._bot_corners(path, robot_width, robot_length)
        rows, n = cor.shape[:2]
        out = np.zeros((rows, n, 20), np.float64)
        for b, o in enumerate(self.bots):
            out[0, b] = o.record()
            for t in range(1, rows):
                c = cor[t, b]
                nm = generate_norm(c)
                r = out[t, b]
                r[0], r[1], r[2] = path[t, b, 0], o.pos[1], path[t, b, 1]
                r[3] = o.safety_radius
                r[4:12] = c.reshape(-1)
                r[12:16] = nm.reshape(-1)
                for a in range(2):
                    r[16 + 2 * a:18 + 2 * a] = _proj(c, nm[a])
        return out

    def bot_render_records(self, path, robot_width=ROBOT_WIDTH, robot_length=ROBOT_LENGTH):
        """[rows, n, 8] float32 (dt_render_bots): render_table's formula in
        float64 on bot_records' corners, rounded once."""
        cor = self._bot_corners(path, robot_width, robot_length)
        c0, e1, e2 = cor[:, :, 0], cor[:, :, 1] - cor[:, :, 0], cor[:, :, 3] - cor[:, :, 0]
        rec = np.concatenate([c0, e1, e2,
                              (e1[..., 0] * e1[..., 0] + e1[..., 1] * e1[..., 1])[..., None],
                              (e2[..., 0] * e2[..., 0] + e2[..., 1] * e2[..., 1])[..., None]], -1)
        return rec.astype(np.float32)

    @property
    def walker_table(self):
        """[K, 5] float64, a row per object_table row (dt_set_walkers): hx, hz,
        vel, W, K; a static row is all zero."""
        recs = [[*o.heading, o.vel, float(o.W), float(o.K)] if o.walker else [0.0] * 5
                for o in self._collidables()]
        return np.array(recs, np.float64).reshape(-1, 5)

    @property
    def render_walker_table(self):
        """[M, 4] float32, a row per render_table row (dt_render_walkers):
        float32(vel * hx), float32(vel * hz), W, K -- the products in float64,
        rounded once; a static row is all zero."""
        recs = [[o.vel * o.heading[0], o.vel * o.heading[1], float(o.W), float(o.K)]
                if o.walker else [0.0] * 4 for o in (self.objects or [])]
        return np.array(recs, np.float64).reshape(-1, 4).astype(np.float32)

    @property
    def spawn_table(self):
        """[M, 4] float64 (x, y, z, radius) of every object (dt_map.spawn_objects)."""
        recs = [np.r_[o.pos, o.spawn_radius] for o in (self.objects or [])]
        return np.array(recs, np.float64).reshape(-1, 4)

    @property
    def render_table(self):
        """[M, 8] float32 footprint records of every object, spawn_table's set
        (dt_render_objects, include/dtsim.h): corner 0 (x, z), e1 = corner 1 -
        corner 0, e2 = corner 3 - corner 0, e1.e1, e2.e2 -- computed in
        float64 from MapObject.corners (the rectangle the collision test uses;
        not norms: a square footprint's eigenvector axes are arbitrary) and
        rounded once."""
        recs = []
        for o in (self.objects or []):
            c = np.asarray(o.corners, np.float64)
            e1, e2 = c[1] - c[0], c[3] - c[0]
            recs.append([c[0, 0], c[0, 1], e1[0], e1[1], e2[0], e2[1],
                         e1[0] * e1[0] + e1[1] * e1[1], e2[0] * e2[0] + e2[1] * e2[1]])
        return np.array(recs, np.float64).reshape(-1, 8).astype(np.float32)

    @property
    def drivable(self):
        return np.nonzero(self.kind > 0)[0]


def tile_curves(kind, orient, i, j, tile_size):
    """upstream _get_curve for one drivable tile."""
    pts = LANE_TEMPLATES[kind] * tile_size
    centre = np.array([(i + .5) * tile_size, 0, (j + .5) * tile_size])
    if kind == TILE_4WAY:
        sides = []
        for rot in np.arange(0, 4):
            side = np.matmul(pts, rotation_y(rot * math.pi / 2))
            side += centre
            sides.append(side)
        return np.reshape(np.array(sides), (12, 4, 3))
    pts = np.matmul(pts, rotation_y(int(orient) * math.pi / 2))
    pts += centre
    return pts


def _parse_entry(d, tile_size, frame_rate, lane_bots):
    if d.get('static', True):
        return parse_object(d, tile_size)
    if lane_bots and d['kind'] == 'duckiebot':
        return parse_bot(d, tile_size)
    return parse_walker(d, tile_size, frame_rate)


def parse_rows(rows, name='custom', tile_size=0.61, objects=(), frame_rate=DEFAULT_FRAMERATE,
               lane_bots=False):
    H, W = len(rows), len(rows[0])
    kind = np.full(H * W, TILE_EMPTY, np.int8)
    orient = np.zeros(H * W, np.int8)
    per_tile = [None] * (H * W)
    for j, row in enumerate(rows):
        if len(row) != W:
            raise ValueError('each row of tiles must have the same length')
        for i, tile in enumerate(row):
            tile = tile.strip()
            t = j * W + i
            if tile == 'empty':
                continue
            if '/' in tile:
                k, o = (s.strip(' ') for s in tile.split('/'))
                if k not in KIND_CODES:
                    raise NotImplementedError('tile kind %r' % k)
                kind[t] = KIND_CODES[k]
                orient[t] = ['S', 'E', 'N', 'W'].index(o)
            elif '4' in tile:        # upstream: kind '4way', angle 2
                kind[t] = TILE_4WAY
                orient[t] = 2
            else:
                kind[t] = TILE_OFFROAD
                continue
            per_tile[t] = tile_curves(int(kind[t]), orient[t], i, j, tile_size)
    counts = [0 if c is None else len(c) for c in per_tile]
    curve_start = np.zeros(H * W + 1, np.int32)
    curve_start[1:] = np.cumsum(counts)
    C = int(curve_start[-1])
    curves = np.zeros((C, 4, 3), np.float64)
    headings = np.zeros((C, 3), np.float64)
    for t, pts in enumerate(per_tile):
        if pts is None:
            continue
        a, b = curve_start[t], curve_start[t + 1]
        curves[a:b] = pts
        h = pts[:, -1, :] - pts[:, 0, :]          # closest_curve_point: one Frobenius norm
        headings[a:b] = h / np.linalg.norm(h).reshape(1, -1)
    objs = [_parse_entry(d, tile_size, frame_rate, lane_bots) for d in objects]
    for o in objs:   # _collidable_object: static, not a traffic light, meets a drivable tile
        if o.kind == 'trafficlight' or not o.static:   # (a walker, a bot: always collidable)
            continue
        for (ti, tj) in find_candidate_tiles(o.corners, tile_size):
            if 0 <= ti < W and 0 <= tj < H and kind[tj * W + ti] > 0 and sat_intersects(
                    o.corners, o.norms, tile_corners(ti, tj, tile_size),
                    np.array([[1.0, 0.0], [0.0, 1.0]])):
                o.collidable = True
                break
    return TileMap(name, W, H, tile_size, kind, orient, curves, headings, curve_start,
                   [list(r) for r in rows], objs)


def load_map(name_or_path, tile_size=0.61, frame_rate=DEFAULT_FRAMERATE, lane_bots=False):
    """lane_bots: load `kind: duckiebot` entries with `static: false` as
    lane-following bots (parse_bot); off, such an entry is refused."""
    path = name_or_path
    if not os.path.exists(path):
        path = os.path.join(MAP_DIR, name_or_path + '.yaml')
    with open(path) as f:
        doc = yaml.safe_load(f)
    objects = doc.get('objects') or []
    if isinstance(objects, dict):   # newer map format: named objects
        objects = list(objects.values())
    name = os.path.splitext(os.path.basename(path))[0]
    return parse_rows(doc['tiles'], name, tile_size, objects, frame_rate, lane_bots)


def _has_bots(path):
    with open(path) as f:
        objects = yaml.safe_load(f).get('objects') or []
    if isinstance(objects, dict):
        objects = list(objects.values())
    return any(d.get('kind') == 'duckiebot' and not d.get('static', True) for d in objects)


def available_maps(lane_bots=False):
    """The shipped maps that load_map(name, lane_bots=lane_bots) loads: a map
    with lane-following bots is listed only with the switch."""
    names = sorted(os.path.splitext(f)[0] for f in os.listdir(MAP_DIR) if f.endswith('.yaml'))
    return [n for n in names
            if lane_bots or not _has_bots(os.path.join(MAP_DIR, n + '.yaml'))]
