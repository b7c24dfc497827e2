"""What one CnnRollout.step() costs on the GPU, by device events
(profiles/cnn_rollout.txt):

    python tools/cnn_rollout_cost.py [--envs 1024] [--steps 30] [--warmup 5]
                                     [--replay {host,device}] [--collect-cost]

A decision's phases are timed by CnnRollout.timer (an event pair around each
launch group): the actor with the action choice, the three steps, the four
renders, the takes and the resets; the step as a whole by one event pair
around it.  collect()'s host time (ReplayBuffer.add_batch: the eviction draws
and the scatter's enqueue) is a host clock around that call, with the device
drained before and after.

--replay device collects into a cnn_replay.CnnReplay instead (the slots
claimed on the device, the decision's takes writing the ring's bytes into
them): there is no add_batch to time, so it reports what --collect-cost adds
for either store: a host clock and an event pair around step() and around
collect(), each from a drained device (host ms: the call returns; drained
ms: the device is idle again; device ms: the events), and collect()'s wall
time a decision over an undrained loop.  collect() minus step() is what
storing adds.
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
    ap.add_argument('--replay', choices=('host', 'device'), default='host',
                    help='host: ddpg.ReplayBuffer.add_batch; device: cnn_replay.CnnReplay')
    ap.add_argument('--collect-cost', action='store_true',
                    help='also time step() and collect() whole (always on with --replay device)')
    args = ap.parse_args()
    from aido1_amd.actor import ActorCNN
    from aido1_amd.cnn_rollout import CnnRollout
    from aido1_amd.ddpg import ReplayBuffer
    dev = torch.device('cuda', 0)
    ro = CnnRollout(ActorCNN(2, 1.0).to(dev), args.envs, map_name=args.map, start_timesteps=0,
                    device=0)
    if args.replay == 'device':
        from aido1_amd.cnn_replay import CnnReplay
        buf = CnnReplay(args.buffer, device=dev)
    else:
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
    if args.replay == 'host':
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
    if args.replay == 'device' or args.collect_cost:
        res['replay'] = args.replay
        res['buffer'] = args.buffer
        res['buffer_len'] = len(buf)
        for name, fn in (('step', ro.step), ('collect', lambda: ro.collect(buf))):
            host = full = device = 0.0
            for _ in range(args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record()
                fn()
                b.record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                host += t1 - t0
                full += time.perf_counter() - t0
                device += a.elapsed_time(b)
            res[name + '_host_ms'] = host * 1e3 / args.steps
            res[name + '_drained_ms'] = full * 1e3 / args.steps
            res[name + '_device_ms'] = device / args.steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ro.collect(buf)
        torch.cuda.synchronize()
        res['collect_wall_ms'] = (time.perf_counter() - t0) * 1e3 / args.steps
    ro.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
