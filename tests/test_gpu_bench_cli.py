"""bench.py's plain run and --dump-outputs on the GPU, at 256 envs: the plain
line carries the headline figure alone (no parity / roofline / sub-records,
those are behind --full), --steps sets the timed decisions, and two runs with
the same arguments dump the same arrays."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ('reward', 'reward_mod', 'done', 'obs', 'state_x', 'state_z', 'state_angle',
         'state_step_count', 'state_env_step', 'state_episode', 'sample_envs', 'frames', 'masks')


def run(capsys, *argv):
    import bench
    bench.main(['--gpus', '1', '--envs', '256'] + list(argv))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_and_dump(gpu, capsys, tmp_path):
    K = 7    # not a multiple of the render group: a trailing single launch
    dirs = [str(tmp_path / 'a'), str(tmp_path / 'b')]
    for d in dirs:
        line = run(capsys, '--steps', str(K), '--warmup', '2', '--dump-outputs', d,
                   '--dump-envs', '8')
        assert line['steps'] == K and line['counts']['decisions'] == K * 256
        assert line['ms_per_step'] == pytest.approx(line['counts']['elapsed_s'] / K * 1e3)
        assert line['value'] == pytest.approx(line['counts']['env_steps'] /
                                              line['counts']['elapsed_s'])
        assert line['higher_is_better'] is True and line['unit'] == 'env-steps/s'
        assert line['full'] is False
        for k in ('parity', 'roofline', 'cpu_baseline', 'config2', 'config4', 'config5'):
            assert k not in line
    assert sorted(os.listdir(dirs[0])) == sorted(n + '.npy' for n in NAMES)
    total = 0
    for n in NAMES:
        a = np.load(os.path.join(dirs[0], n + '.npy'))
        b = np.load(os.path.join(dirs[1], n + '.npy'))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64e6
    fr = np.load(os.path.join(dirs[0], 'frames.npy'))
    mk = np.load(os.path.join(dirs[0], 'masks.npy'))
    assert fr.shape == (8, 3, 120, 160) and mk.shape == (8, 4, 120, 160)
    assert fr.max() > 0 and set(np.unique(mk)) <= {0.0, 255.0} and mk.max() == 255.0
    assert np.load(os.path.join(dirs[0], 'reward.npy')).shape == (256,)


def test_full_run_checks_the_timed_decisions(gpu, capsys):
    line = run(capsys, '--steps', '4', '--warmup', '2', '--full', '--no-lane', '--no-sub',
               '--cpu-steps', '0', '--cpu-procs', '1')
    assert line['full'] is True
    assert line['parity']['ok'] and line['parity']['decisions'] == 4
    assert line['parity']['of'] == 'the timed decisions'
    assert line['roofline']['kernel'] == 'render_kernel' and line['roofline']['frac'] > 0
