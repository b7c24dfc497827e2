"""Batched rollout for duckietown_rl's own DDPG (train-ddpg-cnn.py).

The reference's second consumer of the env contract runs ONE env through
``Simulator`` and host wrappers.  Here one decision of its loop
(train-ddpg-cnn.py:108-140) runs for n envs at once on the device:

  * the observation is ``ImgStacker``'s (duckietown_rl/wrappers.py:54-76): the
    frames of the last three *Simulator steps*, newest first, every slot the
    reset frame after a reset -- so a decision renders each of its REPEAT = 3
    sub-steps, and a terminal ``next_state`` holds fewer new frames when the
    episode ends mid-decision (:122-127 break at ``done``);
  * the action is uniform in the action space during the warm-up, else the
    actor's output plus Gaussian noise, clipped (:109-118);
  * ``repeat_reward``, the ``env_timesteps`` cap and ``done_float`` are the
    script's (:121-139); ``evaluate_policy`` is duckietown_rl/utils.py:60-77.

``SubstepBook`` states the bookkeeping and the action choice with torch ops
(any device); ``FusedBook`` runs the same three steps as the HIP kernels
dt_explore_gauss, dt_substep_account and dt_decision_account
(include/dtactor.h), bit for bit.  ``decide`` / ``evaluate`` are the loops
themselves, written against a small "world" (step, render, take, reset) so
that tests drive them over the reference's own scripted run
(tests/golden/ddpg_cnn_loop.json); ``CnnRollout`` is the world of a VecEnv.
``collect`` stores a decision in a ddpg.ReplayBuffer (float32 stacks, host
eviction draws) or in a cnn_replay.CnnReplay (the ring's bytes, on the device).

Random numbers: one torch generator on the rollout's device.  A ``step()``
draws, in this order and only when used, ``rand(n, 2)`` float64 for the envs
still in the warm-up, then ``randn(n, 2)`` float64 for the others (after
their actor forward, whose dropout has its own counter-based key).
"""
import contextlib
import ctypes

import torch

from aido1_amd import _lib
from aido1_amd.actor import FusedActor
from aido1_amd.camera import resolve as resolve_camera
from aido1_amd.config import EnvConfig
from aido1_amd.render import H, W, RenderOutput

REPEAT = 3          # duckietown_rl/config.py REPEAT
U32_MAX = 0xFFFFFFFF


class SubstepBook:
    """The script's per-decision bookkeeping and action choice for n envs,
    as torch ops on any device.

    State (device tensors, updated in place): ``alive`` u8 (the env has not
    ended inside the current decision), ``repeat_reward`` f64, ``died`` u8
    [3, n] (row r: the envs sub-step r ended), ``episode_timesteps`` i32, and
    ``decision()``'s outputs ``done`` u8, ``done_float`` f32, ``capped`` u8."""

    def __init__(self, n, env_timesteps=500, expl_noise=0.1, low=-1.0, high=1.0, device='cpu'):
        self.n = int(n)
        self.env_timesteps = int(env_timesteps)
        self.expl_noise, self.low, self.high = float(expl_noise), float(low), float(high)
        self.device = dev = torch.device(device)
        self.alive = torch.ones(n, dtype=torch.uint8, device=dev)
        self.repeat_reward = torch.zeros(n, dtype=torch.float64, device=dev)
        self.died = torch.zeros(REPEAT, n, dtype=torch.uint8, device=dev)
        self.episode_timesteps = torch.zeros(n, dtype=torch.int32, device=dev)
        self.done = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.done_float = torch.zeros(n, dtype=torch.float32, device=dev)
        self.capped = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.masks = torch.zeros(2, n, dtype=torch.uint8, device=dev)   # decide()'s unions

    def gauss_actions(self, actor_out, normals, uni, n_warm, out=None):
        """train-ddpg-cnn.py:109-118.  Envs [0, n_warm) take the uniform
        action (float)(low + (high - low) * u); the others
        (float)clip(double(actor_out) + expl_noise * normal, low, high).
        actor_out f32 [n, 2], normals / uni f64 [n, 2] (either may be None
        where no env uses it)."""
        n, lo, hi = self.n, self.low, self.high
        if out is None:
            out = torch.empty(n, 2, dtype=torch.float32, device=self.device)
        if n_warm < n:
            v = actor_out[n_warm:].double() + self.expl_noise * normals[n_warm:]
            out[n_warm:] = v.clamp(lo, hi).float()
        if n_warm > 0:
            out[:n_warm] = (lo + (hi - lo) * uni[:n_warm]).float()
        return out

    def substep(self, reward, done, r, first=None):
        """After sub-step r's Simulator step (:122-127): where alive,
        repeat_reward += reward, died[r] = done, alive &= !done; elsewhere
        died[r] = 0 (the step's entries of an unstepped env are stale).
        first (default r == 0) sets alive = 1 and repeat_reward = 0 before."""
        if first is None:
            first = r == 0
        if first:
            self.alive.fill_(1)
            self.repeat_reward.zero_()
        al = self.alive.bool()
        self.repeat_reward.copy_(torch.where(al, self.repeat_reward + reward, self.repeat_reward))
        d = al & (done != 0)
        self.died[r].copy_(d)
        self.alive.copy_(al & ~d)

    def decision(self):
        """After the last sub-step (:131-139): episode_timesteps += 1; done =
        !alive | (episode_timesteps >= env_timesteps); done_float = 0 where
        episode_timesteps + 1 == env_timesteps, else done; capped = alive &
        done; episode_timesteps = 0 where done."""
        t = self.episode_timesteps + 1
        al = self.alive.bool()
        dn = ~al | (t >= self.env_timesteps)
        self.done.copy_(dn)
        self.done_float.copy_(torch.where(t + 1 == self.env_timesteps,
                                          torch.zeros_like(self.done_float), dn.float()))
        self.capped.copy_(al & dn)
        self.episode_timesteps.copy_(torch.where(dn, torch.zeros_like(t), t))


class FusedBook(SubstepBook):
    """SubstepBook's three steps as one HIP launch each (include/dtactor.h);
    the same state tensors, the same results bit for bit
    (tests/test_gpu_cnn_rollout.py)."""

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def gauss_actions(self, actor_out, normals, uni, n_warm, out=None):
        n = self.n
        if out is None:
            out = torch.empty(n, 2, dtype=torch.float32, device=self.device)
        for t, dt in ((actor_out, torch.float32), (normals, torch.float64), (uni, torch.float64)):
            assert t is None or (t.dtype == dt and t.is_contiguous() and tuple(t.shape) == (n, 2))
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n, 2)
        ptr = (lambda t: t.data_ptr() if t is not None else None)
        _lib.call('dt_explore_gauss', n, int(n_warm), ptr(actor_out), ptr(normals), ptr(uni),
                  self.expl_noise, self.low, self.high, out.data_ptr(), self._stream())
        return out

    def substep(self, reward, done, r, first=None):
        n = self.n
        assert reward.dtype == torch.float64 and done.dtype == torch.uint8
        assert reward.is_contiguous() and done.is_contiguous() and reward.numel() == n == done.numel()
        _lib.call('dt_substep_account', n, int(r == 0 if first is None else first),
                  reward.data_ptr(), done.data_ptr(), self.alive.data_ptr(),
                  self.repeat_reward.data_ptr(), self.died[r].data_ptr(), self._stream())

    def decision(self):
        _lib.call('dt_decision_account', self.n, self.env_timesteps, self.alive.data_ptr(),
                  self.episode_timesteps.data_ptr(), self.done.data_ptr(),
                  self.done_float.data_ptr(), self.capped.data_ptr(), self._stream())


def decide(book, world, actions, state, next_state):
    """One decision of train-ddpg-cnn.py:120-139 for every env of `world`.

    world.take(mask, out): the stack (newest first) of the envs in mask (None:
    all) into out's rows; world.step(alive, actions) -> (reward, done), one
    Simulator step of the envs in alive (None: all), other entries stale;
    world.render(fresh, again=False): every env's current frame into the next
    ring slot (again: the slot of the last render once more), every slot for
    the envs in fresh; world.reset(mask).

    No render is masked.  An unstepped env re-renders its unchanged pose: its
    stack was taken when it died, and after its reset every slot holds the
    reset frame (ImgStacker.reset), which the re-renders repeat.  The last
    render rewrites the same slot with the same bytes for every env that was
    not reset.  So the global newest-first order at sub-step r is each env's
    own for as long as it lives."""
    world.take(None, state)                    # old_obs
    for r in range(REPEAT):
        reward, done = world.step(book.alive if r else None, actions)
        book.substep(reward, done, r)
        world.render(book.died[r - 1] if r else None)
        mask = book.died[r]
        if r == REPEAT - 1:                    # the survivors' next_state too
            mask = torch.bitwise_or(book.died[r], book.alive, out=book.masks[0])
        world.take(mask, next_state)
        world.reset(book.died[r])
    book.decision()
    world.reset(book.capped)
    world.render(torch.bitwise_or(book.died[REPEAT - 1], book.capped, out=book.masks[1]),
                 again=True)


def evaluate(book, world, policy, max_timesteps=1000):
    """duckietown_rl/utils.py:60-77 with one env an episode: every env of
    `world` is reset and runs one episode of at most max_timesteps decisions
    with policy() -> actions [n, 2] f32 (no noise); an ended env is neither
    stepped nor reset.  Returns the sum of all raw rewards divided by the
    number of episodes (each env's rewards are added in order, then the envs'
    sums).  Synchronises once a decision."""
    world.reset(None)
    world.render(None, restart=True)
    for t in range(int(max_timesteps)):
        if t and not bool(book.alive.any()):
            break
        actions = policy()
        for r in range(REPEAT):
            first = t == 0 and r == 0
            reward, done = world.step(None if first else book.alive, actions)
            book.substep(reward, done, r, first=first)
            world.render(None)
    if int(max_timesteps) < 1:
        return 0.0
    return float(book.repeat_reward.sum().item()) / book.n


class CnnRollout:
    """n_envs copies of train-ddpg-cnn.py's env loop on one device.

    policy_or_actor: a ddpg.DDPG (its ``actor``) or an ActorCNN; it acts
    through a FusedActor(float32, mode='reference'): DDPG.predict never calls
    .eval(), so BatchNorm normalises each observation by its own statistics
    and the dropout is live.  ``refresh()`` re-derives the acting weights
    after training.  camera: VecEnv's (default 'ego', the forward camera the
    script's Simulator shows, with launch_env's lens distortion); frames: the ring's 'index' (palette bytes,
    decoded on the fly) or 'gray' frames.  The env is launch_env()'s
    (duckietown_rl/env.py:7-17) under the script's wrappers: steering
    actions, one Simulator step a launch, no wrapper cap, no auto-reset."""

    def __init__(self, policy_or_actor, n_envs, map_name='loop_empty', camera='ego',
                 expl_noise=0.1, start_timesteps=1000, env_timesteps=500, seed=123, device=0,
                 frames='index', draw_objects=False, lane_bots=False):
        from aido1_amd.vec_env import VecEnv
        self.n = int(n_envs)
        self.device = torch.device('cuda', device) if isinstance(device, int) \
            else torch.device(device)
        self.config = EnvConfig(map_name=map_name, repeat_actions=1, max_env_steps=U32_MAX,
                                action_mode='steering', auto_reset=False)
        # launch_env() builds its Simulator with distortion=True (env.py:15):
        # 'ego' is the distorted forward view, as Simulator(camera='ego') gives
        self._env_kw = dict(seed=seed, device=self.device.index or 0, config=self.config,
                            draw_objects=draw_objects, lane_bots=lane_bots,
                            camera=resolve_camera(camera, distortion=True))
        self.frames = frames
        self.env = VecEnv(self.n, **self._env_kw)
        self.out = RenderOutput(self.n, self.device, slots=3, masks=False, frames=frames)
        self.actor_src = getattr(policy_or_actor, 'actor', policy_or_actor).to(self.device)
        self.actor = FusedActor(self.actor_src, dtype=torch.float32, mode='reference')
        self.expl_noise = float(expl_noise)
        self.start_timesteps = int(start_timesteps)
        self.book = FusedBook(self.n, env_timesteps, expl_noise, device=self.device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed))
        self.collected = 0          # transitions so far (the script's total_timesteps)
        kw = dict(dtype=torch.float32, device=self.device)
        self.state = torch.zeros(self.n, 3, H, W, **kw)
        self.next_state = torch.zeros(self.n, 3, H, W, **kw)
        self.action = torch.zeros(self.n, 2, **kw)
        self.timer = None           # tools/cnn_rollout_cost.py: {phase: [(start, end) events]}
        self._eval = None
        self._world = _EnvWorld(self, self.env, self.out)
        self.reset()

    def reset(self):
        """Every env starts an episode (the script's first pass through :100-106)."""
        self._world.reset(None)
        self._world.render(None, restart=True)
        self.book.episode_timesteps.zero_()

    def refresh(self):
        self.actor.refresh(self.actor_src)

    def order(self):
        """Ring slots newest first: ImgStacker's channel order."""
        return self._world.order()

    def stack(self, out=None):
        """The observation every env's next decision acts on: [n, 3, 120, 160]
        float32, newest first (a dt_stack_take of every env)."""
        if out is None:
            out = torch.empty_like(self.state)
        self._world.take(None, out)
        return out

    def _phase(self, name):
        if self.timer is None:
            return contextlib.nullcontext()
        return _Timed(self.timer.setdefault(name, []))

    def step(self, actions=None):
        """One decision for every env.  actions: None (the script's choice:
        uniform in the warm-up, else actor + noise) or a float32 [n, 2]
        tensor.  Returns the device tensors (state, next_state, action,
        repeat_reward, done_float), valid until the next call: both stacks
        [n, 3, 120, 160] float32 newest first, action float32 [n, 2],
        repeat_reward float64 (the sub-steps' raw rewards added in order),
        done_float float32."""
        self._choose(actions)
        decide(self.book, self._world, self.action, self.state, self.next_state)
        self.collected += self.n
        return self.state, self.next_state, self.action, self.book.repeat_reward, \
            self.book.done_float

    def _choose(self, actions):
        """The decision's actions into self.action (step()'s first half)."""
        n, book = self.n, self.book
        if actions is None:
            n_warm = min(n, max(0, self.start_timesteps - self.collected))
            uni = normals = out = None
            with self._phase('actor'):
                if n_warm > 0:
                    uni = torch.rand(n, 2, dtype=torch.float64, device=self.device,
                                     generator=self.gen)
                if n_warm < n:
                    out = self.actor(self.out.ring, self.order())
                    normals = torch.randn(n, 2, dtype=torch.float64, device=self.device,
                                          generator=self.gen)
                book.gauss_actions(out, normals, uni, n_warm, out=self.action)
        else:
            self.action.copy_(actions)

    def collect(self, replay_buffer, actions=None):
        """One decision (actions as step()'s) into a replay buffer.

        A ddpg.ReplayBuffer: step(), then the n transitions in env order
        (add_batch: the reference's eviction draws, on the host); returns
        step()'s tensors.  A cnn_replay.CnnReplay: the slots are claimed
        first and the decision's own takes write the ring's bytes into them
        (dt_stack_store), so no float32 stack is produced; then the scalars;
        returns the claimed rows (int64 [n], -1 where a later transition of
        the batch evicted this one)."""
        from aido1_amd.cnn_replay import CnnReplay
        if not isinstance(replay_buffer, CnnReplay):
            tr = self.step(actions)
            replay_buffer.add_batch(*tr)
            return tr
        if self.frames != 'index':
            raise ValueError("CnnReplay stores the ring's palette-index bytes: a rollout built "
                             "with frames=%r collects into a ddpg.ReplayBuffer" % (self.frames,))
        self._choose(actions)
        rows = replay_buffer.claim(self.n)
        decide(self.book, _StoreWorld(self._world, replay_buffer), self.action, 0, 1)
        replay_buffer.commit(self.action, self.book.repeat_reward, self.book.done_float)
        self.collected += self.n
        return rows

    def evaluate_policy(self, max_timesteps=1000, eval_episodes=10, env_id_base=None):
        """duckietown_rl/utils.py:60-77, batched: eval_episodes envs of their
        own (global ids from env_id_base, default past the collecting envs')
        run one episode each with the acting weights and no noise.  Returns
        the average episode return, as the reference does."""
        e = int(eval_episodes)
        base = self.n if env_id_base is None else int(env_id_base)
        if self._eval is None or self._eval[0] != (e, base):
            from aido1_amd.vec_env import VecEnv
            env = VecEnv(e, env_id_base=base, **self._env_kw)
            out = RenderOutput(e, self.device, slots=3, masks=False, frames=self.frames)
            book = FusedBook(e, self.book.env_timesteps, 0.0, device=self.device)
            self._eval = ((e, base), env, out, book, _EnvWorld(self, env, out))
        _, _env, out, book, world = self._eval
        return evaluate(book, world, lambda: self.actor(out.ring, world.order()), max_timesteps)

    def close(self):
        self.env.close()
        if self._eval is not None:
            self._eval[1].close()
            self._eval = None


class _Timed:
    """Device events around a phase (CnnRollout.timer)."""

    def __init__(self, sink):
        self.sink = sink

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.b = torch.cuda.Event(enable_timing=True)
        self.a.record()

    def __exit__(self, *exc):
        self.b.record()
        self.sink.append((self.a, self.b))


class _EnvWorld:
    """decide()'s world on a VecEnv and its 3-slot ring."""

    def __init__(self, owner, env, out):
        self.owner, self.env, self.out = owner, env, out

    def order(self):
        s = self.out.slot
        return [s % 3, (s - 1) % 3, (s - 2) % 3]

    def take(self, mask, dst):
        o = (ctypes.c_int32 * 3)(*self.order())
        ring = self.out.ring
        with self.owner._phase('take'):
            _lib.call('dt_stack_take', ring.data_ptr(), int(ring.dtype == torch.uint8),
                      self.env.n, self.out.slots, o,
                      mask.data_ptr() if mask is not None else None, dst.data_ptr(),
                      self.env._stream())

    def step(self, alive, actions):
        with self.owner._phase('step'):
            o = self.env.step_into(actions, mask=alive)
        return o.reward, o.done

    def render(self, fresh, again=False, restart=False):
        if restart:
            self.out.restart()
        elif again:     # render_into advances: step back to land on the same slot
            self.out.slot = (self.out.slot - 1) % self.out.slots
        with self.owner._phase('render'):
            self.env.render_into(self.out, fresh=fresh)

    def reset(self, mask):
        env = self.env
        with self.owner._phase('reset'):
            env._check(env._L.dt_reset(env._h, mask.data_ptr() if mask is not None else None,
                                       env._stream()), 'dt_reset')


class _StoreWorld:
    """An _EnvWorld whose take(mask, half) writes the ring's bytes into a
    CnnReplay's claimed rows (half 0: state, 1: next_state) instead of
    decoding them into a float32 stack; step, render and reset are the
    world's own."""

    def __init__(self, world, replay):
        self.world, self.replay = world, replay
        self.step, self.render, self.reset = world.step, world.render, world.reset

    def take(self, mask, half):
        with self.world.owner._phase('take'):
            self.replay.store(self.world.out.ring, self.world.order(), mask, half)
