"""The batched train-ddpg-cnn.py decision (aido1_amd/cnn_rollout.py) against
the reference's own run of that script over a scripted env and policy
(tests/golden/ddpg_cnn_loop.json, written by tests/golden/make_golden_cnn.py):
cnn_rollout.decide / evaluate with SubstepBook's torch bookkeeping, over a
world that plays the fixture's schedule, reproduce every stored transition
(the frame tags of both stacks, the action, repeat_reward, done_float) and
every evaluation return exactly."""
import subprocess

import numpy as np
import pytest
import torch

from conftest import golden

NEW_SYMBOLS = ['dt_explore_gauss', 'dt_substep_account', 'dt_decision_account', 'dt_stack_take']


class ScriptWorld:
    """decide()'s world over the fixture's scripted episodes: env i plays the
    episodes plan[i] one after the other (a reset starts the next one).  A
    frame is its tag, 100 * episode + steps taken; the ring is [n, 3] tags.
    step() writes the entries of the stepped envs only, as dt_step_masked."""

    def __init__(self, episodes, plan):
        self.episodes, self.plan = episodes, [list(p) for p in plan]
        self.n = n = len(plan)
        self.ep, self.k = [None] * n, [0] * n
        self.ring = torch.full((n, 3), -1, dtype=torch.int64)
        self.slot = -1
        self.reward = torch.full((n,), float('nan'), dtype=torch.float64)
        self.done = torch.full((n,), 1, dtype=torch.uint8)      # stale entries say "done"
        self.steps = 0

    def _mask(self, mask):
        return range(self.n) if mask is None else [i for i in range(self.n) if int(mask[i])]

    def order(self):
        return [self.slot % 3, (self.slot - 1) % 3, (self.slot - 2) % 3]

    def take(self, mask, out):
        for i in self._mask(mask):
            out[i] = self.ring[i, self.order()]

    def step(self, alive, actions):
        for i in self._mask(alive):
            r, d = self.episodes[self.ep[i]][self.k[i]]      # past an episode's done: IndexError
            self.k[i] += 1
            self.reward[i], self.done[i] = r, int(d)
            self.steps += 1
        return self.reward, self.done

    def render(self, fresh, again=False, restart=False):
        if restart:
            self.slot, fresh = 0, torch.ones(self.n, dtype=torch.uint8)
        elif not again:
            self.slot = (self.slot + 1) % 3
        for i in range(self.n):
            tag = 100 * self.ep[i] + self.k[i]
            if fresh is not None and int(fresh[i]):
                self.ring[i] = tag
            else:
                self.ring[i, self.slot] = tag

    def reset(self, mask):
        for i in self._mask(mask):
            self.ep[i], self.k[i] = self.plan[i].pop(0), 0


@pytest.fixture(scope='module')
def fx():
    return golden('ddpg_cnn_loop.json')


def _decision_of(episodes, state_tag):
    """(episode, steps before the decision) of a transition's newest old frame."""
    return divmod(state_tag, 100)


def test_fixture_covers_the_schedule(fx):
    """The recorded run holds a death on each of sub-steps 0, 1 and 2, a cap
    ending, and the decision before the cap (done_float forced to 0) both
    with and without a real done."""
    T = fx['args']['env_timesteps']
    died_on, cap_only, before_cap = set(), 0, set()
    for t in fx['train']['transitions']:
        ep, k0 = divmod(t['state'][0], 100)
        steps = fx['episodes'][ep]
        taken = t['next_state'][0] - t['state'][0]
        real_done = steps[k0 + taken - 1][1]
        decision = k0 // 3 + 1                       # 1-based episode_timesteps
        assert k0 % 3 == 0 and 1 <= taken <= 3
        if real_done:
            died_on.add(taken - 1)
        if decision == T and not real_done:
            cap_only += 1
            assert t['done_float'] == 1.0
        if decision + 1 == T:
            before_cap.add(bool(real_done))
            assert t['done_float'] == 0.0
    assert died_on == {0, 1, 2}
    assert cap_only >= 1
    assert before_cap == {True, False}
    assert any(e['max_timesteps'] < 4 for e in fx['evaluations'])     # a truncated evaluation


def test_substep_book_reproduces_the_script(fx):
    """decide() + SubstepBook, one env, fed the training run's schedule and
    draws: every stored transition exactly."""
    from aido1_amd.cnn_rollout import SubstepBook, decide
    a = fx['args']
    tr = fx['train']
    first = tr['first_episode']
    world = ScriptWorld(fx['episodes'], [list(range(first, first + tr['resets'] + 1))])
    book = SubstepBook(1, a['env_timesteps'], a['expl_noise'], fx['action_low'],
                       fx['action_high'])
    world.reset(None)
    world.render(None, restart=True)
    state = torch.zeros(1, 3, dtype=torch.int64)
    next_state = torch.zeros(1, 3, dtype=torch.int64)
    for i, t in enumerate(tr['transitions']):
        warm = i < a['start_timesteps']
        assert warm == ('uniform' in t)
        uni = torch.tensor([t['uniform']], dtype=torch.float64) if warm else None
        out = None if warm else torch.tensor([t['actor_out']], dtype=torch.float32)
        z = None if warm else torch.tensor([t['normal']], dtype=torch.float64)
        act = book.gauss_actions(out, z, uni, 1 if warm else 0)
        # the one stated deviation: the script's float64 action, rounded once
        assert np.array_equal(act.numpy()[0], np.asarray(t['action'], np.float64).astype(np.float32))
        decide(book, world, act, state, next_state)
        assert state[0].tolist() == t['state'], i
        assert next_state[0].tolist() == t['next_state'], i
        assert float(book.repeat_reward[0]) == t['repeat_reward'], i
        assert float(book.done_float[0]) == t['done_float'], i
    # the run's Simulator steps, none taken by a dead env
    assert world.steps == sum(t['next_state'][0] - t['state'][0] for t in tr['transitions'])


def test_batched_evaluation_reproduces_the_script(fx):
    """evaluate(): eval_episodes envs, one episode each, against
    evaluate_policy's sequential return (dyadic rewards: exact in any order)."""
    from aido1_amd.cnn_rollout import SubstepBook, evaluate
    assert fx['script_evaluations'] == [e['return'] for e in fx['evaluations'][:2]]
    for ev in fx['evaluations']:
        n, first = ev['eval_episodes'], ev['first_episode']
        world = ScriptWorld(fx['episodes'], [[first + i] for i in range(n)])
        book = SubstepBook(n, fx['args']['env_timesteps'], 0.0)
        acts = torch.zeros(n, 2)
        got = evaluate(book, world, lambda: acts, ev['max_timesteps'])
        assert got == ev['return'], ev
        assert all(not p for p in world.plan)          # one reset an env, none after its end


def test_ctypes_table_declares_the_new_symbols():
    """_lib.bind's table and include/dtactor.h declare every new entry point,
    and the built library exports them."""
    from aido1_amd import _lib
    declared = _lib.exported_symbols()
    path = _lib.build()
    nm = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True,
                        check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if ' T ' in line}

    class Probe:
        """Records which names bind() sets a signature on."""

        def __init__(self):
            self.bound = {}

        def __getattr__(self, name):
            if not name.startswith('dt_'):
                raise AttributeError(name)
            return self.bound.setdefault(name, type('F', (), {})())
    probe = _lib.bind(Probe())
    for s in NEW_SYMBOLS:
        assert s in declared and s in exported, s
        assert probe.bound[s].restype is not None and len(probe.bound[s].argtypes) >= 8, s
