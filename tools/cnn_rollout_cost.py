"""What one CnnRollout.step() costs on the GPU, by device events
(profiles/cnn_rollout.txt):

    python tools/cnn_rollout_cost.py [--envs 1024] [--steps 30] [--warmup 5]

A decision's phases are timed by CnnRollout.timer (an event pair around each
launch group): the actor with the action choice, the three steps, the four
renders, the takes and the resets; the step as a whole by one event pair
around it.  collect()'s host time (ReplayBuffer.add_batch: the eviction draws
and the scatter's enqueue) is a host clock around that call, with the device
drained before and after.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--map', default='loop_empty')
    ap.add_argument('--buffer', type=int, default=2048)
    args = ap.parse_args()
    from aido1_amd.actor import ActorCNN
    from aido1_amd.cnn_rollout import CnnRollout
    from aido1_amd.ddpg import ReplayBuffer
    dev = torch.device('cuda', 0)
    ro = CnnRollout(ActorCNN(2, 1.0).to(dev), args.envs, map_name=args.map, start_timesteps=0,
                    device=0)
    buf = ReplayBuffer(args.buffer, device=dev)
    for _ in range(args.warmup):
        ro.collect(buf)
    torch.cuda.synchronize()
    ro.timer = {}
    whole = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ro.step()
        b.record()
        whole.append((a, b))
    torch.cuda.synchronize()
    res = {'envs': args.envs, 'steps': args.steps, 'map': args.map,
           'decision_ms': sum(a.elapsed_time(b) for a, b in whole) / args.steps}
    for name, pairs in sorted(ro.timer.items()):     # actor, render, reset, step, take
        res['phase_' + name + '_ms'] = sum(a.elapsed_time(b) for a, b in pairs) / args.steps
        res['phase_' + name + '_launches'] = len(pairs) // args.steps
    ro.timer = None
    # the same loop without the phase events: the events' own cost
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ro.step()
    torch.cuda.synchronize()
    res['decision_wall_ms_untimed'] = (time.perf_counter() - t0) * 1e3 / args.steps
    host, full = 0.0, 0.0
    for _ in range(args.steps):
        tr = ro.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        buf.add_batch(*tr)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        host += t1 - t0
        full += time.perf_counter() - t0
    res['collect_add_batch_host_ms'] = host * 1e3 / args.steps
    res['collect_add_batch_drained_ms'] = full * 1e3 / args.steps
    ro.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
