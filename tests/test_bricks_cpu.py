"""Bricks on the host (no GPU): the C restatement (mt_bricks_*_host) against the numpy restatement written
from the header's text (tests/bricks_ref.py) in random play and from crafted states that force every
event of the rule, the game's invariants, shard == union, controllability (a scripted tracker against the
uniform-random policy), the reference's runner contract, and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import bricks_cases
import bricks_ref
from manette_amd import _lib, bricks

TAB11 = np.arange(11, dtype=np.int32)
TAB1 = np.zeros(1, dtype=np.int32)
SEED = 0x1234567
CONFIGS = [(1, 6, 0), (3, 500, 4)]


def _state_tuple(s):
    return tuple(int(getattr(s, n)) for n in bricks_ref.FIELDS)


def _make_state(t):
    s = _lib.mt_bricks_state()
    for n, v in zip(bricks_ref.FIELDS, t):
        setattr(s, n, int(v))
    return s


@pytest.mark.parametrize('depth', [1, 3])
@pytest.mark.parametrize('lives,max_nexts,serve_wait', CONFIGS)
@pytest.mark.parametrize('R', [1, 11])
def test_host_matches_numpy(depth, lives, max_nexts, serve_wait, R):
    """State records, rewards, over flags, push counts, frames and stacked states, bit for bit: 3 envs under
    uniform-random actions (R = 1, or the table 0..10). The run must have served by fire and by time-out,
    lost lives, ended by lives and by the cap, and ended in the middle of a macro-step."""
    cfg = bricks.config(lives, max_nexts, serve_wait)
    tab = TAB1 if R == 1 else TAB11
    C4 = 4 * depth
    rs = np.random.RandomState(7 + R)
    seen = dict(fire=0, timeout=0, life=0, by_lives=0, by_cap=0, mid=0)
    steps = 110 if R == 1 else 40
    for env in range(3):
        g = bricks_ref.Game(SEED, 100 + env, depth, lives, max_nexts, serve_wait)
        ref_obs = bricks_ref.stack(np.zeros((84, 84, C4), np.uint8), g.new_game(), depth)
        st = _lib.mt_bricks_state()
        obs = np.zeros((84, 84, C4), np.uint8)
        bricks.host_reset(cfg, SEED, 100 + env, depth, st, obs)
        assert _state_tuple(st) == g.state()
        np.testing.assert_array_equal(obs, ref_obs)
        for step in range(steps):
            a, r = int(rs.randint(4)), int(rs.randint(R))
            before = g.state()
            frames_ref, rw_ref, over_ref = g.macro_step(a, int(tab[r]) + 1)
            ref_obs = bricks_ref.stack(ref_obs, frames_ref, depth)
            out = np.empty_like(obs)
            frames = np.zeros((4, 84, 84, depth), np.uint8)
            rw, over, cnt = bricks.host_step(cfg, SEED, 100 + env, depth, tab, a, r, st, obs, out, frames)
            assert (rw, over, cnt) == (float(rw_ref), over_ref, min(len(frames_ref), 4)), (env, step)
            assert _state_tuple(st) == g.state(), (env, step)
            np.testing.assert_array_equal(frames[:cnt], np.asarray(frames_ref[-4:]))
            np.testing.assert_array_equal(out, ref_obs)
            obs = out
            parked_before = before[4] == 0
            if parked_before and g.counter > before[11]:
                seen['fire' if a == 1 else 'timeout'] += 1
            if over:
                # (what ended it: replay the macro-step on a copy, without the new game)
                h = bricks_ref.Game(SEED, 100 + env, depth, lives, max_nexts, serve_wait)
                h.load(before)
                n = 0
                for n in range(1, int(tab[r]) + 2):
                    if h.next(a, render=False)[2]:
                        break
                seen['by_lives' if h.lives == 0 else 'by_cap'] += 1
                seen['mid'] += n < int(tab[r]) + 1
            elif g.lives < before[5]:
                seen['life'] += 1
    assert seen['by_lives'] + seen['by_cap'] > 0, seen
    if (lives, max_nexts, serve_wait) == (1, 6, 0):
        assert seen['by_cap'] > 0 and seen['timeout'] > 0, seen
        if R == 11:
            assert seen['mid'] > 0, seen
    else:
        assert seen['fire'] > 0 and seen['timeout'] > 0 and seen['life'] > 0 and seen['by_lives'] > 0, seen


def _case_cfg():
    return bricks.config(3, 500, 4)


@pytest.mark.parametrize('case', bricks_cases.CASES, ids=[c[0] for c in bricks_cases.CASES])
@pytest.mark.parametrize('depth', [1, 3])
def test_crafted_states(case, depth):
    """Each crafted state forces its event in the first next(): the outcome the rule's text gives, and host
    == numpy over two macro-steps (states, frames, stacked states)."""
    name, state, a, reward, expect = case
    cfg = _case_cfg()
    st = _make_state(state)
    g = bricks_ref.Game(SEED, 9, depth)
    g.load(state)
    obs = np.random.RandomState(3).randint(0, 256, (84, 84, 4 * depth)).astype(np.uint8)
    ref_obs = obs.copy()
    for step in range(2):
        frames_ref, rw_ref, over_ref = g.macro_step(a, 1)
        ref_obs = bricks_ref.stack(ref_obs, frames_ref, depth)
        out = np.empty_like(obs)
        frames = np.zeros((4, 84, 84, depth), np.uint8)
        rw, over, cnt = bricks.host_step(cfg, SEED, 9, depth, TAB1, a, 0, st, obs, out, frames)
        assert (rw, over, cnt) == (float(rw_ref), over_ref, min(len(frames_ref), 4)), step
        assert _state_tuple(st) == g.state(), step
        np.testing.assert_array_equal(frames[:cnt], np.asarray(frames_ref[-4:]))
        np.testing.assert_array_equal(out, ref_obs)
        obs = out
        if step == 0:
            assert rw == reward
            got = dict(zip(bricks_ref.FIELDS, _state_tuple(st)))
            got['bricks'] = got['bricks_lo'] | (got['bricks_hi'] << 64)
            assert {k: got[k] for k in expect} == expect
            first = frames[0]
    # what a frame shows of a brick that the next() broke (gray 90 + 20 r; RGB row colours, red channel)
    row5 = 190 if depth == 1 else 66
    row4 = 170 if depth == 1 else 72
    if name == 'bit76_subframe4':   # broken in sub-frame 4: the render after sub-frame 3 still has it
        assert first[32, 40, 0] == row5 and frames[0][32, 40, 0] == 0
    if name == 'bit63_subframe3':   # broken in sub-frame 3: in neither render
        assert first[28, 42, 0] == 0 and first[28, 41, 0] == row4
    if name == 'last_brick_refills':  # the maximum of the lone brick's render and the refilled wall's
        assert first[32, 40, 0] == row5 and first[17, 3, 0] == (90 if depth == 1 else 200)


@pytest.mark.parametrize('lives,max_nexts,serve_wait', CONFIGS + [(2, 40, 2)])
def test_invariants(lives, max_nexts, serve_wait):
    cfg = bricks.config(lives, max_nexts, serve_wait)
    rs = np.random.RandomState(11)
    for env in range(3):
        st = _lib.mt_bricks_state()
        bricks.host_reset(cfg, SEED, env, 1, st)
        assert st.serve_counter == 0
        length, episodes, counter = 0, 0, 0
        for step in range(1500):
            r = int(rs.randint(11))
            rw, over, cnt = bricks.host_step(cfg, SEED, env, 1, TAB11, int(rs.randint(4)), r, st)
            assert 0 <= rw <= 4 * (r + 1) and rw == int(rw)
            assert 0 <= st.paddle_x <= 68 and 0 <= st.ball_x <= 82 and 0 <= st.ball_y <= 77
            assert st.ball_dx in (-2, -1, 0, 1, 2) and st.ball_dy in (-2, 0, 2)
            assert 1 <= st.lives <= lives and 0 <= st.nexts < max_nexts and 0 <= st.wait <= serve_wait
            assert st.bricks_hi < (1 << 20) and (st.bricks_lo or st.bricks_hi) and st.reserved == 0
            if st.ball_dy == 0:
                assert (st.ball_x, st.ball_y, st.ball_dx) == (st.paddle_x + 7, 77, 0)
            assert st.serve_counter >= counter  # never reset, not by a new game either
            counter = st.serve_counter
            if over:
                assert cnt == 4 and st.nexts == 0 and st.lives == lives and st.ball_dy == 0
                assert (st.bricks_lo, st.bricks_hi) == ((1 << 64) - 1, (1 << 20) - 1)
                length, episodes = 0, episodes + 1
            else:
                length += r + 1
                assert length == st.nexts <= max_nexts and cnt == min(4, r + 1)
        assert episodes >= 1 and counter >= episodes  # (every episode that ended had served at least once)


def _args(argv):
    import train
    return train.get_arg_parser().parse_args(argv)


def test_shard_equals_union():
    """Envs [0, 8) of one creator == envs [0, 4) of a creator at offset 0 and of one at offset 4."""
    from manette_amd.environment_creator import EnvironmentCreator
    union = _args(['-g', 'bricks', '--seed', '5'])
    hi = _args(['-g', 'bricks', '--seed', '5'])
    hi.env_id_offset = 4
    cu, ch = EnvironmentCreator(union), EnvironmentCreator(hi)
    whole = [cu.create_environment(i) for i in range(8)]
    parts = [cu.create_environment(i) for i in range(4)] + [ch.create_environment(i) for i in range(4)]
    for i, (x, y) in enumerate(zip(whole, parts)):
        np.testing.assert_array_equal(x.get_initial_state(), y.get_initial_state())
        for step in range(30):
            a, _ = bricks_ref.hashed_actions(step, 0, 1)  # the same actions for every env: only the serves differ
            ox, rx, dx = x.next(a)
            oy, ry, dy = y.next(a)
            assert (rx, dx) == (ry, dy)
            np.testing.assert_array_equal(ox, oy)
    # and the envs differ from one another (a serve hashes the global env id)
    assert len({_state_tuple(e.state) for e in whole}) > 1


def _tracker(st, rs):
    """fire while parked, otherwise move when the ball's centre is more than 3 px from the paddle's."""
    if st.ball_dy == 0:
        return 1
    d = (st.ball_x + 1) - (st.paddle_x + 8)
    return 2 if d > 3 else (3 if d < -3 else 0)


def _play(cfg, env, policy, episodes, seed=0):
    st = _lib.mt_bricks_state()
    bricks.host_reset(cfg, SEED, env, 1, st)
    rs = np.random.RandomState(seed)
    out, ret = [], 0.0
    while len(out) < episodes:
        rw, over, _ = bricks.host_step(cfg, SEED, env, 1, TAB1, policy(st, rs), 0, st)
        ret += rw
        if over:
            out.append(ret)
            ret = 0.0
    return out


def test_game_is_controllable():
    """100 episodes each at the defaults: the scripted tracker's mean return is at least 10 x the
    uniform-random policy's, which is above 0 (the game can be lost, and it can be controlled); a noop
    paddle scores nothing it does not get from the serves' own bounces."""
    cfg = bricks.config()
    tracker = float(np.mean(_play(cfg, 7, _tracker, 100)))
    random = float(np.mean(_play(cfg, 7, lambda st, rs: int(rs.randint(4)), 100, seed=12345)))
    print('tracker %.2f  random %.2f' % (tracker, random))
    assert random > 0
    assert tracker >= 10 * random


@pytest.mark.parametrize('lives,max_nexts,serve_wait', CONFIGS)
def test_runner_contract(lives, max_nexts, serve_wait):
    """BricksEmulator under the reference-contract runner loop == mt_bricks_step_host driven directly."""
    from manette_amd.emulator_runner import run_emulators
    E = 3
    cfg = bricks.config(lives, max_nexts, serve_wait)
    emus = [bricks.BricksEmulator(10 + e, seed=SEED, lives=lives, max_nexts=max_nexts, serve_wait=serve_wait)
            for e in range(E)]
    states = np.asarray([e.get_initial_state() for e in emus])
    variables = [states, np.zeros(E, np.float32), np.zeros(E, np.float32), np.zeros(E, np.int32), np.zeros(E, np.int32)]
    sts = [_lib.mt_bricks_state() for _ in range(E)]
    obs = [np.zeros((84, 84, 4), np.uint8) for _ in range(E)]
    for e in range(E):
        bricks.host_reset(cfg, SEED, 10 + e, 1, sts[e], obs[e])
        np.testing.assert_array_equal(states[e], obs[e])
    ended = 0
    for step in range(60):
        for e in range(E):
            variables[3][e], variables[4][e] = bricks_ref.hashed_actions(step, e, 11)
        run_emulators(list(TAB11), emus, variables)
        for e in range(E):
            out = np.empty_like(obs[e])
            rw, over, _ = bricks.host_step(cfg, SEED, 10 + e, 1, TAB11, variables[3][e], variables[4][e], sts[e],
                                           obs[e], out)
            obs[e] = out
            ended += over
            assert (variables[1][e], bool(variables[2][e])) == (rw, over), (step, e)
            np.testing.assert_array_equal(variables[0][e], out)
            assert _state_tuple(emus[e].state) == _state_tuple(sts[e])
    assert ended > 0


def test_argument_checks():
    import train
    from manette_amd.environment_creator import DEVICE_GAMES, EnvironmentCreator
    from manette_amd.paac import check_arch_flags
    assert DEVICE_GAMES == ('catch', 'bricks')
    ec = EnvironmentCreator(_args(['-g', 'bricks', '--bricks_lives', '2', '--bricks_max_nexts', '9',
                                   '--bricks_serve_wait', '1']))
    assert ec.num_actions == 4
    emu = ec.create_environment(0)
    assert isinstance(emu, bricks.BricksEmulator)
    assert (emu.cfg.lives, emu.cfg.max_nexts, emu.cfg.serve_wait) == (2, 9, 1)
    assert EnvironmentCreator(_args(['-g', 'breakout'])).create_environment(0).__class__.__name__ == 'SyntheticEmulator'
    train.validate_args(_args(['-g', 'bricks', '--runner', 'device', '--arch', 'NIPS']))
    train.validate_args(_args(['-g', 'bricks', '--runner', 'python', '--arch', 'LSTM']))
    with pytest.raises(ValueError, match='catch.*bricks'):
        train.validate_args(_args(['-g', 'breakout', '--runner', 'device', '--arch', 'NIPS']))
    with pytest.raises(ValueError, match='LSTM'):
        check_arch_flags(_args(['-g', 'bricks', '--runner', 'device', '--arch', 'LSTM']))
    with pytest.raises(ValueError, match='bayes_native'):
        check_arch_flags(_args(['-g', 'bricks', '--runner', 'device', '--arch', 'BAYESIAN', '--bayes_native']))
    with pytest.raises(ValueError, match='native runner'):
        check_arch_flags(_args(['-g', 'bricks', '--runner', 'native']))
    # the C ABI's own checks: before anything runs
    lib = _lib.hip()
    st = _lib.mt_bricks_state()
    rw, ov = C.c_float(), C.c_float()
    tab = TAB1.ctypes.data_as(C.c_void_p)
    for cfg, depth in ((bricks.config(0, 500, 4), 1), (bricks.config(3, 0, 4), 1), (bricks.config(3, 500, -1), 1),
                       (bricks.config(), 2)):
        assert lib.mt_bricks_reset_host(C.byref(cfg), 0, 0, depth, C.byref(st), None) == 1
        assert lib.mt_bricks_step_host(C.byref(cfg), 0, 0, depth, tab, 1, 0, 0, C.byref(st), None, None, None, None,
                                       C.byref(rw), C.byref(ov)) == 1
    ok = bricks.config()
    assert lib.mt_bricks_reset_host(C.byref(ok), 0, 0, 1, None, None) == 1
    assert lib.mt_bricks_step_host(C.byref(ok), 0, 0, 1, tab, 0, 0, 0, C.byref(st), None, None, None, None,
                                   C.byref(rw), C.byref(ov)) == 1  # R < 1
    obs = np.zeros((84, 84, 4), np.uint8)
    p = obs.ctypes.data_as(C.c_void_p)
    assert lib.mt_bricks_step_host(C.byref(ok), 0, 0, 1, tab, 1, 0, 0, C.byref(st), p, p, None, None,
                                   C.byref(rw), C.byref(ov)) == 1  # out aliases prev
    for args in ((C.byref(ok), 0, 0, 0, 1, None, None, None), (C.byref(ok), 0, -1, 4, 1, None, None, None),
                 (C.byref(ok), 0, 0, 4, 2, None, None, None), (None, 0, 0, 4, 1, None, None, None)):
        assert lib.mt_bricks_reset(*args) == 1  # (refused before any launch: no GPU is touched)
    assert lib.mt_bricks_step(C.byref(ok), 0, 0, 4, 1, None, 1, None, None, None, None, None, None, None, None, None,
                              None, 0, 5, None) == 1


def test_out_of_range_indices_are_clamped():
    cfg = bricks.config()
    for (a, r), (ac, rc) in (((-5, -1), (0, 0)), ((9, 99), (3, 10)), ((1, 3), (1, 3)), ((4, 10), (3, 10))):
        s1, s2 = _lib.mt_bricks_state(), _lib.mt_bricks_state()
        bricks.host_reset(cfg, SEED, 1, 1, s1)
        bricks.host_reset(cfg, SEED, 1, 1, s2)
        assert bricks.host_step(cfg, SEED, 1, 1, TAB11, a, r, s1) == bricks.host_step(cfg, SEED, 1, 1, TAB11, ac, rc, s2)
        assert _state_tuple(s1) == _state_tuple(s2)
        assert bricks_ref.clamp_indices(a, r, 11) == (ac, rc)


def test_statistics_run_needs_no_frame_pointers():
    """NULL frame pointers: the same states, rewards and flags, nothing rendered."""
    cfg = bricks.config(1, 6, 0)
    s1, s2 = _lib.mt_bricks_state(), _lib.mt_bricks_state()
    obs = np.zeros((84, 84, 4), np.uint8)
    bricks.host_reset(cfg, SEED, 3, 1, s1, obs)
    bricks.host_reset(cfg, SEED, 3, 1, s2)
    for step in range(60):
        a, r = bricks_ref.hashed_actions(step, 3, 11)
        out = np.empty_like(obs)
        got1 = bricks.host_step(cfg, SEED, 3, 1, TAB11, a, r, s1, obs, out)
        got2 = bricks.host_step(cfg, SEED, 3, 1, TAB11, a, r, s2)
        assert got1 == got2 and _state_tuple(s1) == _state_tuple(s2)
        obs = out
