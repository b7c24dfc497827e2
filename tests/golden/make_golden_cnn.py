"""Generate tests/golden/ddpg_cnn_loop.json by RUNNING the reference's
train-ddpg-cnn.py (and its duckietown_rl/utils.py evaluate_policy) over a
scripted env and a scripted policy.

    python tests/golden/make_golden_cnn.py [/path/to/reference]

Nothing of the reference's text is copied: the script file is executed
(runpy) with its collaborators injected through sys.modules --

  * ``gym``: the Wrapper base classes and spaces.Box the reference's own
    duckietown_rl/wrappers.py builds on (its ImgStacker, ImgTransposer,
    ActionWrapper, ... run unchanged);
  * ``scipy.misc.imresize`` / ``skimage.color.rgb2gray``: stand-ins that keep a
    frame's tag (ResizeWrapper blows the 2 x 2 frame up to 120 x 160 with the
    same value, GrayscaleWrapper keeps channel 0);
  * ``hyperdash.Experiment``: a no-op;
  * ``duckietown_rl.args``: the arguments below;
  * ``duckietown_rl.env.launch_env``: the scripted env -- episode e is a list
    of (reward, done) per Simulator step, its frames 2 x 2 x 3 arrays filled
    with the tag 100 e + k (k = 0: the reset frame, k: after its k-th step);
  * ``duckietown_rl.ddpg.DDPG``: the scripted policy -- predict() is a fixed
    function of the stack's tags, train / save / load do nothing.

numpy's normal() is wrapped to record the standard normals it draws (the
value it returns is numpy's own loc + scale * z); the env's
action_space.sample() records its uniforms.  The fixture holds the env's
script, every stored transition (the tags of both stacks, the action, the
draws behind it, repeat_reward, done_float) and evaluate_policy's returns.
"""
import argparse
import contextlib
import io
import json
import os
import runpy
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'

ENV_TIMESTEPS = 4
ARGS = dict(seed=3, start_timesteps=3, eval_freq=1e9, max_timesteps=26, save_models=False,
            expl_noise=0.25, batch_size=4, discount=0.99, tau=0.005, policy_noise=0.2,
            noise_clip=0.5, policy_freq=2, env_timesteps=ENV_TIMESTEPS,
            replay_buffer_max_size=10000)
# Simulator steps until each episode's own `done`, in the order the episodes
# start, cycled.  With REPEAT = 3 and env_timesteps = 4 a length L ends the
# episode on sub-step (L - 1) % 3 of decision (L - 1) // 3 + 1: 1, 5 and 9 die
# on sub-steps 0, 1 and 2 (9: in decision 3 = env_timesteps - 1, the decision
# whose done_float is forced to 0, with a real done), 11 dies inside the cap's
# own decision, 20 outlives the cap (decision 3 without a done, then a cap
# ending); 2 and 6 vary the rest.
LENGTHS = [5, 20, 1, 9, 11, 2, 20, 6]


def episode_script(e):
    """Episode e's (reward, done) for every step: dyadic rewards (every sum is
    exact in float64, so the order of additions cannot matter), one -1000 like
    the Simulator's invalid-pose reward."""
    n = LENGTHS[e % len(LENGTHS)]
    steps = []
    for k in range(1, n + 1):
        r = ((7 * e + 3 * k) % 16 - 8) / 4.0
        if k == n and e % 3 == 0:
            r = -1000.0
        steps.append([r, k == n])
    return steps


def install_stubs(log):
    gym = types.ModuleType('gym')

    class Wrapper:
        def __init__(self, env=None):
            self.env = env
            self.observation_space = getattr(env, 'observation_space', None)
            self.action_space = getattr(env, 'action_space', None)

        def reset(self):
            return self.env.reset()

        def step(self, action):
            return self.env.step(action)

    class ObservationWrapper(Wrapper):
        def reset(self):
            return self.observation(self.env.reset())

        def step(self, action):
            obs, reward, done, info = self.env.step(action)
            return self.observation(obs), reward, done, info

    class ActionWrapper(Wrapper):
        def step(self, action):
            return self.env.step(self.action(action))

    class RewardWrapper(Wrapper):
        def step(self, action):
            obs, reward, done, info = self.env.step(action)
            return obs, self.reward(reward), done, info

    class Box:
        def __init__(self, low, high, shape=None, dtype=np.float32):
            self.shape = tuple(shape) if shape is not None else np.shape(low)
            self.low = np.full(self.shape, low, dtype) if np.isscalar(low) else low
            self.high = np.full(self.shape, high, dtype) if np.isscalar(high) else high
            self.dtype = dtype

        def sample(self):
            u = np.random.random(self.shape)
            log['uniforms'].append(u.tolist())
            return (self.low.astype(np.float64) +
                    (self.high.astype(np.float64) - self.low.astype(np.float64)) * u
                    ).astype(np.float32)

    gym.Wrapper, gym.ObservationWrapper = Wrapper, ObservationWrapper
    gym.ActionWrapper, gym.RewardWrapper = ActionWrapper, RewardWrapper
    gym.make = lambda *a, **k: None
    spaces = types.ModuleType('gym.spaces')
    spaces.Box = Box
    gym.spaces = spaces
    sys.modules['gym'] = gym
    sys.modules['gym.spaces'] = spaces

    import scipy
    misc = types.ModuleType('scipy.misc')
    misc.imresize = lambda arr, size: np.full(tuple(size), np.asarray(arr)[0, 0, 0], np.float64)
    sys.modules['scipy.misc'] = misc
    scipy.misc = misc
    sk = types.ModuleType('skimage')
    color = types.ModuleType('skimage.color')
    color.rgb2gray = lambda rgb: np.asarray(rgb, np.float64)[..., 0]
    sk.color = color
    sys.modules['skimage'] = sk
    sys.modules['skimage.color'] = color

    hd = types.ModuleType('hyperdash')

    class Experiment:
        def __init__(self, *a, **k):
            pass

        def metric(self, *a, **k):
            pass

        def end(self):
            pass
    hd.Experiment = Experiment
    sys.modules['hyperdash'] = hd

    class ScriptEnv:
        """Episode e = the e-th reset; see the module docstring."""

        def __init__(self):
            self.observation_space = Box(0, 255, (2, 2, 3), np.uint8)
            self.action_space = Box(-1.0, 1.0, (2,), np.float32)
            self.episode = -1
            self.k = 0

        def _frame(self):
            return np.full((2, 2, 3), 100 * self.episode + self.k, np.float64)

        def reset(self):
            self.episode += 1
            self.k = 0
            self.script = episode_script(self.episode)
            log['resets'] += 1
            return self._frame()

        def step(self, action):
            assert np.asarray(action).shape == (2,)
            reward, done = self.script[self.k]      # stepping past `done` is an error
            self.k += 1
            return self._frame(), reward, done, {}

    the_env = ScriptEnv()
    envmod = types.ModuleType('duckietown_rl.env')
    envmod.launch_env = lambda id=None: the_env
    sys.modules['duckietown_rl.env'] = envmod

    argmod = types.ModuleType('duckietown_rl.args')
    argmod.get_ddpg_args_train = lambda: argparse.Namespace(**ARGS)
    sys.modules['duckietown_rl.args'] = argmod

    class DDPG:
        def __init__(self, state_dim, action_dim, max_action, net_type='cnn'):
            # (state_dim is ImgStacker's declared [3, 1, 120], not its stacks' shape)
            assert action_dim == 2 and max_action == 1.0

        def predict(self, state):
            t = [int(state[c, 0, 0]) for c in range(3)]
            out = policy_out(t)
            log['actor_out'].append(out.tolist())
            return out

        def train(self, *a, **k):
            pass

        def save(self, *a, **k):
            pass

        def load(self, *a, **k):
            raise FileNotFoundError(2, 'no model', 'scripted')
    ddpgmod = types.ModuleType('duckietown_rl.ddpg')
    ddpgmod.DDPG = DDPG
    sys.modules['duckietown_rl.ddpg'] = ddpgmod
    return the_env, DDPG


def policy_out(tags):
    """The scripted actor: a float32 function of the stack's tags, inside the
    head's range (sigmoid | tanh), near enough to its ends for the clip to act."""
    return np.array([(tags[0] % 7) / 6.0, ((tags[0] + 2 * tags[1] + tags[2]) % 9 - 4) / 4.0],
                    np.float32)


def main():
    sys.path.insert(0, REF)
    log = {'uniforms': [], 'normals': [], 'actor_out': [], 'resets': 0, 'evals': []}
    env, DDPG = install_stubs(log)
    import duckietown_rl.utils as ru

    real_normal = np.random.normal

    def normal(loc=0.0, scale=1.0, size=None):
        z = np.random.standard_normal(size)
        log['normals'].append(np.asarray(z).tolist())
        return loc + scale * z          # numpy's own definition of normal()
    real_eval = ru.evaluate_policy

    def evaluate_policy(env_, policy, max_timesteps=1000, eval_episodes=10):
        first, n_pred = log['resets'], len(log['actor_out'])
        ret = real_eval(env_, policy, max_timesteps=max_timesteps, eval_episodes=eval_episodes)
        assert log['resets'] - first == eval_episodes
        del log['actor_out'][n_pred:]       # keep the training loop's predictions only
        log['evals'].append({'first_episode': first, 'eval_episodes': eval_episodes,
                             'max_timesteps': max_timesteps, 'return': float(ret)})
        return ret
    ru.evaluate_policy = evaluate_policy
    np.random.normal = normal
    cwd = os.getcwd()
    try:
        with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
            os.chdir(tmp)
            g = runpy.run_path(os.path.join(REF, 'train-ddpg-cnn.py'), run_name='__main__')
            os.chdir(cwd)
        train_first = log['evals'][0]['first_episode'] + log['evals'][0]['eval_episodes']
        train_resets = log['evals'][1]['first_episode'] - train_first
        # one more evaluation, cut short by max_timesteps, straight from the
        # reference's function on the script's own (wrapped) env
        with contextlib.redirect_stdout(io.StringIO()):
            evaluate_policy(g['env'], g['policy'], max_timesteps=2, eval_episodes=4)
    finally:
        os.chdir(cwd)
        np.random.normal = real_normal
        ru.evaluate_policy = real_eval

    storage = g['replay_buffer'].storage
    assert len(storage) == ARGS['max_timesteps'] and len(log['evals']) == 3
    warm = ARGS['start_timesteps']
    assert len(log['uniforms']) == warm and len(log['normals']) == len(storage) - warm
    assert len(log['actor_out']) == len(storage) - warm
    trans = []
    for i, (state, next_state, action, reward, done) in enumerate(storage):
        tags = [[int(s[c, 0, 0]) for c in range(3)] for s in (state, next_state)]
        assert all(np.all(s[c] == s[c, 0, 0]) for s in (state, next_state) for c in range(3))
        t = {'state': tags[0], 'next_state': tags[1],
             'action': [float(v) for v in np.asarray(action, np.float64)],
             'repeat_reward': float(reward), 'done_float': float(done)}
        if i < warm:
            t['uniform'] = log['uniforms'][i]
        else:
            t['actor_out'] = log['actor_out'][i - warm]
            t['normal'] = log['normals'][i - warm]
        trans.append(t)
    n_episodes = log['resets']
    out = {'repeat': 3, 'args': {k: ARGS[k] for k in ('start_timesteps', 'expl_noise',
                                                      'env_timesteps', 'max_timesteps')},
           'action_low': -1.0, 'action_high': 1.0,
           'episodes': [episode_script(e) for e in range(n_episodes + 1)],
           'train': {'first_episode': train_first, 'resets': train_resets,
                     'transitions': trans},
           'evaluations': log['evals'], 'script_evaluations': [float(v) for v in g['evaluations']]}
    with open(os.path.join(HERE, 'ddpg_cnn_loop.json'), 'w') as f:
        json.dump(out, f, indent=None, separators=(',', ':'))
    print('wrote ddpg_cnn_loop.json: %d transitions, %d episodes' % (len(trans), n_episodes))


if __name__ == '__main__':
    main()
