"""train-ddpg-cnn.py's collect-and-train loop for many envs at once, on
CnnRollout (the collecting half) and CnnReplay (the storing half).

The reference trains at each episode's end for as many DDPG.train iterations
as the episode had timesteps (train-ddpg-cnn.py:100-103): over a run, one
iteration per collected transition.  n envs end their episodes at n
different times, so the batched rule spreads the same ratio evenly:
``iterations_per_decision`` iterations after every collect() (default: n,
one per transition of the decision), once the buffer holds a batch.  Every
training round is followed by rollout.refresh(), so the next decision acts
with the trained weights, as the script's policy object does.
"""


class CnnTrainLoop:
    """policy: a ddpg.DDPG whose ``actor`` the rollout acts with; rollout: a
    CnnRollout(frames='index'); replay: a cnn_replay.CnnReplay on the same
    device.  Nothing in a decision synchronises with the host (pass the
    policy log=None: its progress line is a host print, not a device read)."""

    def __init__(self, policy, rollout, replay, batch_size=32, discount=0.99, tau=0.005,
                 iterations_per_decision=None):
        self.policy, self.rollout, self.replay = policy, rollout, replay
        self.batch_size = int(batch_size)
        self.discount, self.tau = float(discount), float(tau)
        self.iterations_per_decision = rollout.n if iterations_per_decision is None \
            else int(iterations_per_decision)
        if self.batch_size < 1 or self.iterations_per_decision < 0:
            raise ValueError('batch_size >= 1 and iterations_per_decision >= 0')
        self.decisions = self.iterations = self.rounds = 0

    def run(self, decisions):
        """`decisions` times: collect, then (buffer permitting) train and
        refresh.  Returns the running counts: decisions, transitions (the
        rollout's ``collected``), iterations, training rounds."""
        for _ in range(int(decisions)):
            self.rollout.collect(self.replay)
            self.decisions += 1
            if len(self.replay) >= self.batch_size and self.iterations_per_decision:
                self.policy.train(self.replay, self.iterations_per_decision, self.batch_size,
                                  self.discount, self.tau)
                self.iterations += self.iterations_per_decision
                self.rounds += 1
                self.rollout.refresh()
        return {'decisions': self.decisions, 'transitions': self.rollout.collected,
                'iterations': self.iterations, 'rounds': self.rounds}

    def evaluate(self, *args, **kwargs):
        """rollout.evaluate_policy: the average return of fresh episodes under
        the acting weights, without noise."""
        return self.rollout.evaluate_policy(*args, **kwargs)
