"""Diagnostic: config 3's renders one decision a launch (dt_render) against two
and three decisions a launch (dt_render2 / dt_render3), 4096 envs, the poses
and done flags of dt_step_many chunks of 18 decisions; HIP events around each
chunk's renders.  Prints ms per decision for each form (alternating, R rounds).

--map picks the map (default loop_empty); --draw-objects draws its objects,
--lane-bots loads its duckiebots, --camera ego renders the forward camera's
view, --camera identity the top-down frame through the identity table (what
the gather alone costs); both also print the frames' listed-word counts (the
non-uniform words the line detector works on), counted on an index-frame
render of the last poses.  On a handle that draws walkers or bots
(loop_pedestrians, loop_dyn_duckiebots) every form renders each decision at
its own time (dt_step_many_time's output through dt_render_group); elsewhere
the calls are the ones they always were."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aido1_amd.config import EnvConfig  # noqa: E402
from aido1_amd.render import RenderOutput, bind_render, bind_render_group  # noqa: E402
from aido1_amd.vec_env import StepOutput, VecEnv  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
ap.add_argument('--map', default='loop_empty')
ap.add_argument('--draw-objects', action='store_true')
ap.add_argument('--lane-bots', action='store_true')
ap.add_argument('--camera', choices=['ego', 'identity'], default=None)
ap.add_argument('--envs', type=int, default=4096)
ap.add_argument('--rounds', type=int, default=int(os.environ.get('R', '5')))
args = ap.parse_args()

n, k, R = args.envs, 18, args.rounds
# identity: the top-down frame itself through phase 0d (what the gather alone costs)
camera = np.arange(19200, dtype=np.uint16).reshape(120, 160) if args.camera == 'identity' \
    else args.camera
dev = torch.device('cuda', 0)
env = VecEnv(n, seed=1234, device=0, config=EnvConfig(map_name=args.map),
             draw_objects=args.draw_objects, lane_bots=args.lane_bots, camera=camera)
dynamic = env.draw_objects and (env.map.has_walkers or len(env.map.bots) > 0)
env.reset()
ro = RenderOutput(n, dev)
extra = [torch.zeros_like(ro.masks) for _ in range(2)]
g = torch.Generator(device=dev)
g.manual_seed(3)
s = torch.cuda.current_stream(dev)
res = {1: [], 2: [], 3: []}
for r in range(R + 1):
    for form in (1, 2, 3):
        acts = torch.rand(k, n, 2, generator=g, device=dev)
        out = StepOutput(k * n, dev, lanepos=False, tile=False)
        pose = torch.empty(k, 3, n, dtype=torch.float64, device=dev)
        time = torch.empty(k, n, dtype=torch.int32, device=dev) if dynamic else None
        env.step_many_into(acts, out, pose=pose, time=time)
        done = out.done.view(k, n)
        if form == 1:
            calls = [bind_render(env, ro, s, fresh=done[d], pose=pose[d],
                                 time=time[d] if dynamic else None) for d in range(k)]
        else:
            calls = [bind_render_group(env, ro, s, extra[:form - 1],
                                       [done[d + i] for i in range(form)],
                                       [pose[d + i] for i in range(form)],
                                       time=[time[d + i] for i in range(form)] if dynamic else None)
                     for d in range(0, k, form)]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = 0
        for c in calls:
            rc |= c()
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0
        if r:
            res[form].append(e0.elapsed_time(e1) / k)
print('map %s, draw_objects %s, lane_bots %s, camera %s, %d envs%s' % (
    args.map, args.draw_objects, args.lane_bots, args.camera, n,
    ', each decision at its own time' if dynamic else ''))
for form, v in res.items():
    print('%d a launch, ms per decision: %s  mean %.4f' % (form, ' '.join('%.4f' % x for x in v),
                                                  sum(v) / len(v)))
if args.camera:
    # the words the kernel lists (phase 1): a 4-pixel word whose 3 x 6-pixel
    # neighbourhood, edges replicated, is not one palette byte
    io = RenderOutput(n, dev, slots=1, frames='index')
    env.render_into(io, pose=pose[k - 1], time=time[k - 1] if dynamic else None)
    x = torch.nn.functional.pad(io.ring.float(), (1, 1, 1, 1), mode='replicate')
    pool = torch.nn.functional.max_pool2d
    listed = (pool(x, (3, 6), stride=(1, 4)) != -pool(-x, (3, 6), stride=(1, 4))).sum((1, 2, 3))
    print('listed words a frame: median %d  max %d' % (listed.median().item(), listed.max().item()))
