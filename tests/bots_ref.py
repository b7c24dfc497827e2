"""CPU restatement of the lane-following bots (include/dtsim.h, dt_bot_path /
dt_set_bots) on top of the oracle's SimulatorRef: the test reference for
tests/test_bots.py and tests/test_gpu_bots.py.  Nothing under oracle/ knows
about bots.

A bot (`kind: duckiebot`, `static: false`; keys `velocity` m/s >= 0, default
0.1, and `follow_dist` m > 0, default 0.3) starts at home -- pos times the tile
size, angle = radians(rotate) -- and takes one step per Simulator step, float64
in numpy's operation order:

  1. (P, T) = closest_curve_point(pos, angle)            the oracle's own
  2. L = follow_dist; up to 1000 times: F = P + T * L,
     (C, _) = closest_curve_point(F, angle); stop at the first C that exists,
     else L *= 0.5
  3. v = C - pos; v /= |v|; steer = gain * -(right(angle) . v)
  4. wheels: SteeringToWheelVelWrapper.action on (velocity, steer) with gain
     2.0, trim 0.0, radius 0.0318, k 27.0, limit 1.0: k_inv = (gain +- trim)
     / k; w = (vel +- 0.5 * steer * wheel_dist) / radius; u = w * k_inv clamped
     to +-limit; vels = [u_l, u_r]
  5. pose: the oracle's _update_pos(pos, angle, wheel_dist, vels, delta_time),
     vels as given (not multiplied by robot_speed)

The path is undefined (PathUndefined) when 1 finds no curve, 2 ends without a
C, or a value is not finite.  The bot reads nothing of the agent, so its pose
at Simulator step count t is row t of one table for every env; past the table
it stays at the last row (min(t, rows - 1)).

The box: at t = 0 the bot's static record (generate_corners of its mesh
extents); at t >= 1 corners = agent_boundbox(pos_t, ROBOT_WIDTH, ROBOT_LENGTH,
dir(angle_t), right(angle_t)), axes = generate_norm of them, centre = pos_t,
the safety radius unchanged.  Which t: after the counter's increment in
update_physics, 0 in reset.  In the collidable lists the statics come first,
then the walkers (tests/walkers_ref.py: a `duckie` with `static: false` on the
same map), then the bots, each in load order.
"""
import math

import numpy as np

import walkers_ref as WR
from oracle import dtsim_ref as R

BOT_VELOCITY, BOT_FOLLOW_DIST = 0.1, 0.3
GAIN, TRIM, RADIUS, K_MOTOR, LIMIT = 2.0, 0.0, 0.0318, 27.0, 1.0


class PathUndefined(Exception):
    pass


def wheels(vel, steer, wheel_dist=R.WHEEL_DIST, gain=GAIN, trim=TRIM, radius=RADIUS, k=K_MOTOR,
           limit=LIMIT):
    """Stage 4: [u_l, u_r]."""
    k_r_inv = (gain + trim) / k
    k_l_inv = (gain - trim) / k
    omega_r = (vel + 0.5 * steer * wheel_dist) / radius
    omega_l = (vel - 0.5 * steer * wheel_dist) / radius
    u_r = omega_r * k_r_inv
    u_l = omega_l * k_l_inv
    return np.array([max(min(u_l, limit), -limit), max(min(u_r, limit), -limit)])


def bot_step(sim, x, z, angle, velocity, follow_dist):
    """One Simulator step of a bot from (x, z, angle) on sim's map."""
    pos = np.array([x, 0.0, z])
    P, T = sim.closest_curve_point(pos, angle)
    if P is None:
        raise PathUndefined('left the drivable tiles at (%r, %r)' % (x, z))
    L = follow_dist
    C = None
    for _ in range(1000):
        F = P + T * L
        C, _t = sim.closest_curve_point(F, angle)
        if C is not None:
            break
        L *= 0.5
    if C is None:
        raise PathUndefined('no follow point from (%r, %r)' % (x, z))
    v = C - pos
    v = v / R._norm3(v)
    r = R.get_right_vec(angle)
    steer = GAIN * -((r[0] * v[0] + r[1] * v[1]) + r[2] * v[2])
    vels = wheels(velocity, steer, sim.wheel_dist)
    pos, angle = R._update_pos(pos, angle, sim.wheel_dist, vels, sim.delta_time)
    out = (float(pos[0]), float(pos[2]), float(angle))
    if not all(math.isfinite(q) for q in out):
        raise PathUndefined('non-finite pose from (%r, %r)' % (x, z))
    return out


class Bot:
    def __init__(self, desc, tile_size):
        assert desc['kind'] == 'duckiebot' and desc.get('static', True) is False
        pos = desc['pos']
        y = pos[2] if len(pos) == 3 else 0.0
        self.pos = tile_size * np.array((pos[0], y, pos[1]))
        mn = np.array(desc['mesh_min'], np.float64)
        mx = np.array(desc['mesh_max'], np.float64)
        self.scale = desc['height'] / mx[1] if 'height' in desc else desc.get('scale', 1.0)
        self.max_coords = mx
        self.angle = float(np.radians(desc.get('rotate', 0)))
        self.corners = R.generate_corners(self.pos, mn, mx, self.angle, self.scale)
        self.norm = R.generate_norm(self.corners)
        self.safety_radius = R.SAFETY_RAD_MULT * R.calculate_safety_radius(mn, mx, self.scale)
        self.velocity = float(desc.get('velocity', BOT_VELOCITY))
        self.follow_dist = float(desc.get('follow_dist', BOT_FOLLOW_DIST))

    @property
    def home(self):
        return (float(self.pos[0]), float(self.pos[2]), self.angle)

    def box(self, t, pose):
        """(corners, norm, centre) at step t, pose = the table's row."""
        if t == 0:
            return self.corners, self.norm, self.pos
        x, z, a = pose
        centre = np.array([x, self.pos[1], z])
        c = R.agent_boundbox(centre, R.ROBOT_WIDTH, R.ROBOT_LENGTH, R.get_dir_vec(a),
                             R.get_right_vec(a))
        return c, R.generate_norm(c), centre


def split_objects(objects):
    """(statics, bots); walkers_of gives the map's walkers."""
    statics = [d for d in objects if d.get('static', True)]
    bots = [d for d in objects if not d.get('static', True) and d['kind'] == 'duckiebot']
    return statics, bots


def walkers_of(objects):
    return [d for d in objects if not d.get('static', True) and d['kind'] == 'duckie']


def own_path(tiles, objects, rows, cfg=None):
    """[rows, n_bots, 3]: the restatement's paths from home."""
    cfg = cfg or R.SimConfig()
    statics, bots = split_objects(objects)
    sim = R.SimulatorRef(tiles, cfg=cfg, objects=statics)
    bots = [Bot(d, cfg.road_tile_size) for d in bots]
    path = np.zeros((rows, len(bots), 3))
    for b, bot in enumerate(bots):
        path[0, b] = bot.home
        for t in range(rows - 1):
            path[t + 1, b] = bot_step(sim, *path[t, b], bot.velocity, bot.follow_dist)
    return path


class BotSimRef(R.SimulatorRef):
    """SimulatorRef of a map with bots that follow `path` [rows, n_bots, 3]."""

    def __init__(self, map_rows, path, seed=123, env_id=0, cfg=None, objects=(), boxes=None):
        statics, bots = split_objects(objects)
        super().__init__(map_rows, seed, env_id, cfg, statics)
        m = self.map
        self.bots = [Bot(d, self.cfg.road_tile_size) for d in bots]
        self.walkers = [WR.Walker(d, self.cfg.road_tile_size, self.cfg.frame_rate)
                        for d in walkers_of(objects)]
        self.path = np.asarray(path, np.float64)
        assert self.path.shape[1:] == (len(self.bots), 3)
        # (corners, norm, centre) of every row, shared between the envs of a batch
        self.boxes = boxes if boxes is not None else [
            [bot.box(t, self.path[t, b]) for b, bot in enumerate(self.bots)]
            for t in range(len(self.path))]
        # statics first, then the walkers, then the bots
        self.first_walker = len(m.collidable_corners)
        self.first = self.first_walker + len(self.walkers)
        movers = self.walkers + self.bots
        m.collidable_centers = np.concatenate(
            [m.collidable_centers.reshape(-1, 3)] + [w.pos.reshape(1, 3) for w in movers])
        m.collidable_safety_radii = np.concatenate(
            [m.collidable_safety_radii, [w.safety_radius for w in movers]])
        for w in movers:
            m.collidable_corners.append(w.corners.copy())
            m.collidable_norms.append(w.norm)
            m.objects.append({'kind': 'mover', 'pos': w.pos, 'scale': w.scale,
                              'max_coords': w.max_coords, 'corners': w.corners, 'norm': w.norm,
                              'safety_radius': w.safety_radius, 'visible': True})
        self.penalty_negative = False   # set by any negative penalty since it was cleared

    def place(self, t):
        m = self.map
        row = self.boxes[min(int(t), len(self.boxes) - 1)]
        for j, (c, nm, centre) in enumerate(row):
            m.collidable_corners[self.first + j] = c
            m.collidable_norms[self.first + j] = nm
            m.collidable_centers[self.first + j] = centre
        for j, w in enumerate(self.walkers):
            dx, dz = w.shift(t)
            m.collidable_corners[self.first_walker + j] = w.corners + np.array([dx, dz])
            m.collidable_centers[self.first_walker + j] = w.pos + np.array([dx, 0.0, dz])

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

    def hit_a_bot_away_from_home(self):
        """The current pose is invalid, and would be valid with every mover at home."""
        now = self._valid_pose(self.cur_pos, self.cur_angle)
        self.place(0)
        home = self._valid_pose(self.cur_pos, self.cur_angle)
        self.place(self.step_count)
        return home and not now


class BotBatchRef:
    """n envs of EnvironmentWrapperRef(BotSimRef) with VecEnv's auto-reset: a
    finished env respawns and reports its terminal tile."""

    def __init__(self, rows, objects, path, n, seed, **cfg_kw):
        self.objects = objects
        self.cfg = R.SimConfig(**cfg_kw)
        first = BotSimRef(rows, path, seed, 0, self.cfg, objects)
        self.envs = [R.EnvironmentWrapperRef(first)] + [
            R.EnvironmentWrapperRef(BotSimRef(rows, path, seed, e, self.cfg, objects, first.boxes))
            for e in range(1, n)]
        self.n = n
        self.ends = self.bot_ends = self.decisions = self.negative = 0

    def reset(self):
        for w in self.envs:
            w.reset()

    def set_step_count(self, t):
        for w, v in zip(self.envs, t):
            w.sim.step_count = int(v)
            w.sim.place(int(v))

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
                self.bot_ends += bool(w.sim.hit_a_bot_away_from_home())
                w.reset()
        return out

    def state(self):
        return dict(x=np.array([w.sim.cur_pos[0] for w in self.envs]),
                    z=np.array([w.sim.cur_pos[2] for w in self.envs]),
                    angle=np.array([w.sim.cur_angle for w in self.envs]),
                    step_count=np.array([w.sim.step_count for w in self.envs], np.uint32))


# ---- the tests' fixture map -------------------------------------------------------------
# the walkers' loop with three bots at lane centres (0.2 of a tile right of the
# tile's middle line, heading along the lane) and one static cone
BOT = dict(kind='duckiebot', height=0.12, mesh_min=[-0.6, 0.0, -0.45], mesh_max=[0.6, 1.0, 0.45],
           static=False)
FIXTURE_TILES = [['curve_left/W', 'straight/W', 'straight/W', 'curve_left/N'],
                 ['straight/S', 'grass', 'grass', 'straight/N'],
                 ['curve_left/S', 'straight/E', 'straight/E', 'curve_left/E']]
FIXTURE_OBJECTS = [
    dict(BOT, pos=[1.5, 0.3], rotate=180, velocity=0.15),
    dict(kind='cone', pos=[2.5, 2.95], height=0.1, mesh_min=[-0.35, 0.0, -0.35],
         mesh_max=[0.35, 1.0, 0.35]),
    dict(BOT, pos=[2.5, 2.7], rotate=0, velocity=0.3, follow_dist=0.25),
    dict(BOT, pos=[0.3, 1.5], rotate=-90),
]
FIXTURE_ROWS = 1001      # t = 0 .. 1000


def write_map(path, objects=FIXTURE_OBJECTS, tiles=FIXTURE_TILES):
    import yaml
    with open(path, 'w') as f:
        yaml.safe_dump({'tiles': tiles, 'objects': [dict(o) for o in objects]}, f)
    return str(path)


# a walker crossing the top straight and a bot driving along it, one cone: the
# walker + bot paths of the kernels and the frame
MIXED_OBJECTS = [
    dict(BOT, pos=[2.5, 0.3], rotate=180, velocity=0.3),
    dict(WR.DUCKIE, pos=[1.5, 0.05], rotate=-90, static=False, wait=0.1),
    dict(kind='cone', pos=[2.5, 2.95], height=0.1, mesh_min=[-0.35, 0.0, -0.35],
         mesh_max=[0.35, 1.0, 0.35]),
    dict(BOT, pos=[0.3, 1.5], rotate=-90),
]


def all_static(objects):
    """The same objects with every `static: false` removed."""
    return [{k: v for k, v in o.items() if k != 'static'} for o in objects]
