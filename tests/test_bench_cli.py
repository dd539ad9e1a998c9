"""bench.py's command line: a plain run prints the headline line only, --full adds the measurements
that take runs of their own, --steps sets the number of timed steps, and --dump-outputs writes the
last timed step's arrays, identical from run to run (float32, within the size limit)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup')
FULL_ONLY = ('roofline', 'kernels', 'train_pass', 'trunk_isolated', 'rollout_forward', 'profile_windows')
# a short settle phase keeps the runs short (the default with --dump-outputs is 2000 updates)
SHORT = ['--gpus', '1', '--steps', '3', '--warmup', '2', '--settle_updates', '4']


def run_bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(args), cwd=ROOT,
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_write_outputs_float32_and_size_limit(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    rs = np.random.RandomState(3)
    arrays = {'small': rs.randint(0, 9, (5, 7)).astype(np.int32), 'big': rs.randn(4000).astype(np.float64),
              'big2': rs.randn(50, 60).astype(np.float32)}
    # under the limit: every array whole, in float32
    shapes = bench.write_outputs(arrays, str(tmp_path / 'a'), limit_bytes=1 << 20)
    assert shapes == {'small': [5, 7], 'big': [4000], 'big2': [50, 60]}
    for k, x in arrays.items():
        y = np.load(str(tmp_path / 'a' / (k + '.npy')))
        assert y.dtype == np.float32
        np.testing.assert_array_equal(y, x.astype(np.float32))
    # over it: the arrays above their share are cut to the same seeded sample on every call
    limit = 12000
    for d in ('b', 'c'):
        shapes = bench.write_outputs(arrays, str(tmp_path / d), limit_bytes=limit)
    got = {k: np.load(str(tmp_path / 'b' / (k + '.npy'))) for k in arrays}
    assert sum(x.nbytes for x in got.values()) <= limit
    np.testing.assert_array_equal(got['small'], arrays['small'].astype(np.float32))
    assert got['big'].shape == got['big2'].shape == (limit // 12,)
    assert np.isin(got['big'], arrays['big'].astype(np.float32)).all()
    assert shapes == {k: list(x.shape) for k, x in got.items()}
    for k in arrays:
        np.testing.assert_array_equal(got[k], np.load(str(tmp_path / 'c' / (k + '.npy'))))


@pytest.mark.gpu
@pytest.mark.timeout(240)
def test_dump_outputs_identical_from_run_to_run(tmp_path):
    """Two processes with the same arguments: the same inputs, so the same arrays bit for bit; a
    plain run's line holds the headline fields and none of the --full measurements."""
    lines = [run_bench(*SHORT, '--dump-outputs', str(tmp_path / d)) for d in ('a', 'b')]
    for line in lines:
        for k in HEADLINE:
            assert k in line, k
        assert line['steps'] == 3 and line['warmup'] == 2
        assert line['ms_per_step'] > 0 and line['value'] > 0 and line['higher_is_better'] is True
        assert line['config']['settle_updates'] == 4
        # value = env-steps of the timed steps over their time (ec=32, t_max=5 per step)
        assert abs(line['value'] - 160 / (line['ms_per_step'] * 1e-3)) <= 0.01 * line['value']
        assert not [k for k in FULL_ONLY if k in line]
    names = sorted(os.listdir(str(tmp_path / 'a')))
    assert names == sorted(os.listdir(str(tmp_path / 'b')))
    assert {'params.npy', 'grad.npy', 'values.npy', 'pi.npy', 'actions.npy', 'returns.npy'} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(str(tmp_path / 'a' / n)), np.load(str(tmp_path / 'b' / n))
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        np.testing.assert_array_equal(x, y, err_msg=n)
        total += x.nbytes
    assert total <= 64 << 20
    assert lines[0]['dumped_outputs']['shapes']['values'] == [5, 32]
    # the timed steps ran an update: its gradient is not all zero
    assert np.abs(np.load(str(tmp_path / 'a' / 'grad.npy'))).max() > 0


@pytest.mark.gpu
@pytest.mark.timeout(240)
def test_full_adds_the_other_measurements():
    line = run_bench(*SHORT, '--full', '--no_cpu_baseline', '--trunk_sweep=', '--measure_updates', '2')
    for k in HEADLINE + FULL_ONLY:
        assert k in line, k
    assert line['steps'] == 3
    assert line['roofline']['us_per_launch'] > 0
