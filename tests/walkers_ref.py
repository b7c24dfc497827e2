"""CPU restatement of the walkers (include/dtsim.h, dt_set_walkers) on top of
the oracle's SimulatorRef: the test reference for tests/test_walkers.py and
tests/test_gpu_walkers.py.  Nothing under oracle/ knows about walkers.

A walker (`kind: duckie`, `static: false`) stands idx steps of `vel` along its
heading (cos a, -sin a), a = radians(rotate), from home at Simulator step count
t, with W = round(wait * frame_rate), D = walk_distance + 0.25, K the smallest
k >= 1 with float64(k) * vel > D, and

    P = W + K;  leg = t // P;  p = t % P;  m = max(0, p - W)
    idx = m on an even leg, K - m on an odd leg
    s = float64(idx) * vel;  (dx, dz) = (s * hx, s * hz)

Its corners and centre are translated by (dx, dz), one add each; its axes stay.
The map's static objects go through MapRef as they always have; each walker's
home corners, axes, centre and safety radius (the oracle's own
generate_corners / generate_norm / calculate_safety_radius) are appended to
the map's collidable lists (a walker is always collidable) and re-placed from
the step counter: after its increment in update_physics, and at 0 in reset.
"""
import math

import numpy as np

from oracle import dtsim_ref as R

WALKER_VEL, WALKER_WAIT, WALKER_EXTRA = 0.02, 8.0, 0.25


def index_at(t, W, K):
    """The closed form above, restated (aido1_amd.maps.walker_index is the
    product's; tests/test_walkers.py checks both against a step-by-step loop)."""
    P = W + K
    leg, p = t // P, t % P
    m = max(0, p - W)
    return m if leg % 2 == 0 else K - m


def index_by_stepping(t, W, K):
    """The walk itself, a step at a time: wait W steps, walk K, turn, repeat."""
    idx, direction, waited = 0, 1, 0
    for _ in range(t):
        if waited < W:
            waited += 1
            continue
        idx += direction
        if idx == (K if direction > 0 else 0):
            direction, waited = -direction, 0
    return idx


class Walker:
    def __init__(self, desc, tile_size, frame_rate):
        assert desc['kind'] == 'duckie' and desc.get('static', True) is False
        pos = desc['pos']
        y = pos[2] if len(pos) == 3 else 0.0
        self.pos = tile_size * np.array((pos[0], y, pos[1]))
        mn = np.array(desc['mesh_min'], np.float64)
        mx = np.array(desc['mesh_max'], np.float64)
        self.scale = desc['height'] / mx[1] if 'height' in desc else desc.get('scale', 1.0)
        self.max_coords = mx
        a = np.radians(desc.get('rotate', 0))
        self.corners = R.generate_corners(self.pos, mn, mx, a, self.scale)
        self.norm = R.generate_norm(self.corners)
        self.safety_radius = R.SAFETY_RAD_MULT * R.calculate_safety_radius(mn, mx, self.scale)
        self.hx, self.hz = math.cos(a), -math.sin(a)
        self.vel = float(desc.get('vel', WALKER_VEL))
        self.W = int(round(float(desc.get('wait', WALKER_WAIT)) * frame_rate))
        D = float(desc.get('walk_distance', tile_size)) + WALKER_EXTRA
        k = 1
        while not float(k) * self.vel > D:
            k += 1
        self.K = k

    def shift(self, t):
        s = float(index_at(int(t), self.W, self.K)) * self.vel
        return s * self.hx, s * self.hz


def split_objects(objects):
    statics = [d for d in objects if d.get('static', True)]
    walkers = [d for d in objects if not d.get('static', True)]
    return statics, walkers


class WalkerSimRef(R.SimulatorRef):
    """SimulatorRef of a map with walkers."""

    def __init__(self, map_rows, seed=123, env_id=0, cfg=None, objects=()):
        statics, walkers = split_objects(objects)
        super().__init__(map_rows, seed, env_id, cfg, statics)
        m = self.map
        self.walkers = [Walker(d, self.cfg.road_tile_size, self.cfg.frame_rate) for d in walkers]
        self.first = len(m.collidable_corners)     # statics first, then the walkers
        m.collidable_centers = np.concatenate(
            [m.collidable_centers] + [w.pos.reshape(1, 3) for w in self.walkers])
        m.collidable_safety_radii = np.concatenate(
            [m.collidable_safety_radii, [w.safety_radius for w in self.walkers]])
        for w in self.walkers:
            m.collidable_corners.append(w.corners.copy())
            m.collidable_norms.append(w.norm)
            m.objects.append({'kind': 'duckie', 'pos': w.pos, 'scale': w.scale,
                              'max_coords': w.max_coords, 'corners': w.corners, 'norm': w.norm,
                              'safety_radius': w.safety_radius, 'visible': True})
        self.penalty_negative = False   # set by any negative penalty since it was cleared

    def place(self, t):
        m = self.map
        for j, w in enumerate(self.walkers):
            dx, dz = w.shift(t)
            m.collidable_corners[self.first + j] = w.corners + np.array([dx, dz])
            m.collidable_centers[self.first + j] = w.pos + np.array([dx, 0.0, dz])

    def update_physics(self, action, delta_time=None):
        super().update_physics(action, delta_time)
        self.place(self.step_count)

    def reset(self):
        self.place(0)
        return super().reset()

    def proximity_penalty2(self, pos, angle):
        pen = super().proximity_penalty2(pos, angle)
        if pen < 0:
            self.penalty_negative = True
        return pen

    def hit_a_walker_away_from_home(self):
        """The current pose is invalid, and would be valid with every walker at home."""
        now = self._valid_pose(self.cur_pos, self.cur_angle)
        self.place(0)
        home = self._valid_pose(self.cur_pos, self.cur_angle)
        self.place(self.step_count)
        return home and not now


class WalkerBatchRef:
    """n envs of EnvironmentWrapperRef(WalkerSimRef) with VecEnv's auto-reset:
    a finished env respawns and reports its terminal tile."""

    def __init__(self, rows, objects, n, seed, **cfg_kw):
        self.cfg = R.SimConfig(**cfg_kw)
        self.envs = [R.EnvironmentWrapperRef(WalkerSimRef(rows, seed, e, self.cfg, objects))
                     for e in range(n)]
        self.n = n
        self.ends = self.walker_ends = self.decisions = self.negative = 0

    def reset(self):
        for w in self.envs:
            w.reset()

    def set_step_count(self, t):
        for w, v in zip(self.envs, t):
            w.sim.step_count = int(v)
            w.sim.place(int(v))

    def set_pose(self, x, z, angle):
        for w, px, pz, a in zip(self.envs, x, z, angle):
            w.sim.cur_pos = np.array([px, 0.0, pz])
            w.sim.cur_angle = float(a)

    def step(self, actions):
        out = dict(reward=np.zeros(self.n), reward_mod=np.zeros(self.n),
                   done=np.zeros(self.n, np.uint8), tile=np.zeros(self.n, np.int32))
        for e, w in enumerate(self.envs):
            w.sim.penalty_negative = False
            r, rm, done = w.step(actions[e])
            out['reward'][e], out['reward_mod'][e], out['done'][e] = r, rm, done
            out['tile'][e] = w.tile_index()
            self.decisions += 1
            self.negative += bool(w.sim.penalty_negative)
            if done:
                self.ends += 1
                self.walker_ends += bool(w.sim.hit_a_walker_away_from_home())
                w.reset()
        return out

    def state(self):
        return dict(x=np.array([w.sim.cur_pos[0] for w in self.envs]),
                    z=np.array([w.sim.cur_pos[2] for w in self.envs]),
                    angle=np.array([w.sim.cur_angle for w in self.envs]),
                    step_count=np.array([w.sim.step_count for w in self.envs], np.uint32))


# ---- the GPU tests' fixture map ---------------------------------------------------------
DUCKIE = dict(kind='duckie', height=0.08, mesh_min=[-0.5, 0.0, -0.4], mesh_max=[0.5, 1.0, 0.4])
FIXTURE_TILES = [['curve_left/W', 'straight/W', 'straight/W', 'curve_left/N'],
                 ['straight/S', 'grass', 'grass', 'straight/N'],
                 ['curve_left/S', 'straight/E', 'straight/E', 'curve_left/E']]
FIXTURE_OBJECTS = [
    dict(DUCKIE, pos=[1.5, 0.05], rotate=-90, static=False, wait=0.1),
    dict(DUCKIE, pos=[3.95, 1.5], rotate=180, static=False, wait=0.2, vel=0.03),
    dict(kind='cone', pos=[1.5, 2.5], height=0.1, mesh_min=[-0.35, 0.0, -0.35],
         mesh_max=[0.35, 1.0, 0.35]),
    dict(DUCKIE, pos=[0.3, 1.2], rotate=90, static=False, wait=0, walk_distance=0.4),
]


def write_map(path, objects=FIXTURE_OBJECTS, tiles=FIXTURE_TILES):
    import yaml
    with open(path, 'w') as f:
        yaml.safe_dump({'tiles': tiles, 'objects': [dict(o) for o in objects]}, f)
    return str(path)


def all_static(objects):
    """The same objects with every `static: false` removed."""
    return [{k: v for k, v in o.items() if k != 'static'} for o in objects]
