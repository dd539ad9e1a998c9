"""The structured frames of tests/structured_frames.py do reach the exact max-pool ties (oracle only).

Non-vacuity conditions for tests/test_structured_frames_gpu.py, on the frames, batch and initial
weights it uses: enough pool windows of every pooled PWYX layer have four identical receptive
fields, enough of them carry gradient (a positive pooled value), the fp64 oracle itself routes every
one of them to position 0, and parity_util.device_branches' threshold rule alone would hand nearly
all conv1 windows to the device — the blind spot its exact mode closes.
"""
import functools

import numpy as np
import pytest

import structured_frames as sf
from oracle import nets

MIN_SHARE = {'conv1': 0.50, 'conv2': 0.25, 'conv3': 0.10}
CASES = [(depth, act) for depth in (1, 3) for act in ('relu', 'leaky_relu')]


def test_frames_layout():
    for depth in (1, 3):
        x = sf.frames(sf.SEED, sf.B, depth)
        assert x.dtype == np.uint8 and x.shape == (sf.B, 84, 84, 4 * depth)
        assert np.array_equal(x, sf.frames(sf.SEED, sf.B, depth)) and not np.array_equal(x, sf.frames(1, sf.B, depth))
        assert not x[:, 0].any() and (x[:, 1] == 255).all()
        assert len({f.tobytes() for f in x}) == sf.B
        moved = [not np.array_equal(f[..., 0], f[..., 3]) for f in x]
        assert any(moved), 'no rectangle moves between the stacked time steps'
        # planes [p_t0..p_t3]: the background of a plane is one colour over its four time steps
        bg = x[:, 83, 83].reshape(sf.B, depth, 4)
        assert (bg == bg[:, :, :1]).all()


def test_identical_windows_small():
    x = np.zeros((1, 6, 6, 2), np.float32)
    x[0, 2, 2, 1] = 1.0  # a 3x3 field sees it from output rows / cols 1..3
    got = sf.identical_windows(x, 3)
    # SAME zero padding: every field of the constant-0 remainder is identical, borders included
    want = np.ones((1, 3, 3), bool)
    want[0, :2, :2] = False  # windows (rows 0-1 | 2-3) x (cols 0-1 | 2-3) hold an output in 1..3
    assert np.array_equal(got, want)
    ones = np.ones((1, 6, 6, 1), np.uint8)  # a non-zero constant differs from the zero padding at the border
    assert np.array_equal(sf.identical_windows(ones, 3)[0], np.pad(np.ones((1, 1), bool), 1))


@functools.lru_cache(maxsize=None)
def _oracle(depth, act):
    spec = nets.arch_spec('PWYX', depth, 4, 11)
    P = nets.init_params(spec, sf.SEED)
    x = sf.frames(sf.SEED, sf.B, depth)
    _, layers = nets.trunk_forward(spec, P, x, act, 0.1)
    return x, [L for L in layers if L['pool']]


@pytest.mark.parametrize('depth,act', CASES)
def test_identical_windows_are_common_routed_first_and_carry_gradient(depth, act):
    x, layers = _oracle(depth, act)
    inp = x
    for L in layers:
        same = sf.identical_windows(inp, L['k'])
        assert same.mean() >= MIN_SHARE[L['name']], (L['name'], float(same.mean()))
        live = same[..., None] & (L['yp'] > 0)
        assert live.sum() >= 1000, (L['name'], int(live.sum()))
        arg, gap = nets.pool_route(L['y'])
        assert not arg[same].any() and not gap[same].any(), L['name']  # exact ties, first position
        inp = L['yp']


@pytest.mark.parametrize('depth,act', CASES)
def test_threshold_rule_alone_hands_conv1_to_the_device(depth, act):
    """device_branches without exact=True: a window is 'clear' (the device's argmax is compared) only
    when its top two values differ by tie = 1e-5 x the layer's RMS."""
    _, layers = _oracle(depth, act)
    L = layers[0]
    _, gap = nets.pool_route(L['y'])
    tied = gap * np.maximum(np.abs(L['yp']), 1e-30) < 1e-5 * np.sqrt(np.mean(L['y'] ** 2))
    assert tied.all(axis=-1).mean() >= 0.90, float(tied.all(axis=-1).mean())
