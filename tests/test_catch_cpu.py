"""Catch on the host (no GPU): the C restatement (mt_catch_*_host) against the numpy restatement
written from the header's text (tests/catch_ref.py), the game's invariants, shard == union, a scripted
paddle that catches everything (so the learning bar of tests/test_catch_gpu.py is attainable), the
reference's runner contract, and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import catch_ref
from manette_amd import _lib, catch

TAB11 = np.asarray(catch_ref.tab_repetitions(10, 11), dtype=np.int32)
TAB1 = np.zeros(1, dtype=np.int32)
SEED = 0x1234567


def _state_tuple(s):
    return (s.paddle_x, s.ball_x, s.ball_y, s.ball_dx, s.misses, s.balls, s.ball_counter)


@pytest.mark.parametrize('depth', [1, 3])
@pytest.mark.parametrize('lives,max_balls', [(1, 2), (3, 20)])
def test_host_matches_numpy(depth, lives, max_balls):
    """State, reward, over, frames and stacked state, bit for bit: 8 envs, 200 macro-steps of hashed
    actions under the FiGAR table of max_repetition 10, nb_choices 11."""
    cfg = catch.config(lives, max_balls)
    C4 = 4 * depth
    ended = 0
    for env in range(8):
        g = catch_ref.Game(SEED, 100 + env, depth, lives, max_balls)
        ref_obs = catch_ref.stack(np.zeros((84, 84, C4), np.uint8), g.new_game(), depth)
        st = _lib.mt_catch_state()
        obs = np.zeros((84, 84, C4), np.uint8)
        catch.host_reset(cfg, SEED, 100 + env, depth, st, obs)
        assert _state_tuple(st) == g.state()
        np.testing.assert_array_equal(obs, ref_obs)
        for step in range(200):
            a, r = catch_ref.hashed_actions(step, env, 11)
            frames_ref, rw_ref, over_ref = g.macro_step(a, int(TAB11[r]) + 1)
            ref_obs = catch_ref.stack(ref_obs, frames_ref, depth)
            out = np.empty_like(obs)
            frames = np.zeros((4, 84, 84, depth), np.uint8)
            rw, over, cnt = catch.host_step(cfg, SEED, 100 + env, depth, TAB11, a, r, st, obs, out, frames)
            assert (rw, over, cnt) == (float(rw_ref), over_ref, min(len(frames_ref), 4)), (env, step)
            assert _state_tuple(st) == g.state(), (env, step)
            np.testing.assert_array_equal(frames[:cnt], np.asarray(frames_ref[-4:]))
            np.testing.assert_array_equal(out, ref_obs)
            obs = out
            ended += over
    assert ended >= 8  # episodes did end inside the run (inside repeats under lives 1, max_balls 2)


def test_statistics_run_needs_no_frame_pointers():
    """NULL frame pointers: the same states, rewards and flags, nothing rendered."""
    cfg = catch.config(1, 2)
    s1, s2 = _lib.mt_catch_state(), _lib.mt_catch_state()
    obs = np.zeros((84, 84, 4), np.uint8)
    catch.host_reset(cfg, SEED, 3, 1, s1, obs)
    catch.host_reset(cfg, SEED, 3, 1, s2)
    for step in range(60):
        a, r = catch_ref.hashed_actions(step, 3, 11)
        out = np.empty_like(obs)
        got1 = catch.host_step(cfg, SEED, 3, 1, TAB11, a, r, s1, obs, out)
        got2 = catch.host_step(cfg, SEED, 3, 1, TAB11, a, r, s2)
        assert got1 == got2 and _state_tuple(s1) == _state_tuple(s2)
        obs = out


def episode_next_bounds(lives, max_balls):
    """A ball spawns at ball_y = 0 and lands when ball_y = 76: 38 sub-frames later, when the next spawns.
    The new game plays 16 sub-frames before the first next(), so landing k happens 38k - 16 sub-frames
    into the episode: it ends no earlier than landing `lives` and no later than landing `max_balls`."""
    first = -(-(38 * min(lives, max_balls) - 16) // 4)
    last = -(-(38 * max_balls - 16) // 4)
    return first, last


@pytest.mark.parametrize('lives,max_balls', [(1, 2), (3, 20), (2, 5)])
def test_invariants(lives, max_balls):
    cfg = catch.config(lives, max_balls)
    lo, hi = episode_next_bounds(lives, max_balls)
    for env in range(4):
        st = _lib.mt_catch_state()
        catch.host_reset(cfg, SEED, env, 1, st)
        ret, length, episodes = 0.0, 0, 0
        for step in range(1500):
            a, _ = catch_ref.hashed_actions(step, env, 1)
            before = _state_tuple(st)
            rw, over, cnt = catch.host_step(cfg, SEED, env, 1, TAB1, a, 0, st)
            assert rw in (-1.0, 0.0, 1.0)
            assert 0 <= st.paddle_x <= 72 and 0 <= st.ball_x <= 80 and 0 <= st.ball_y <= 76 and st.ball_dx in (-1, 0, 1)
            ret += rw
            length += 1
            assert length <= hi
            if over:
                assert cnt == 4 and -lives <= ret <= max_balls and lo <= length <= hi
                # the state is the next game's initial state: the numpy new game from the same ball counter
                g = catch_ref.Game(SEED, env, 1, lives, max_balls)
                g.counter = before[6]  # (the next that ended the game spawned nothing: its one landing ended it)
                g.new_game(render=False)
                assert _state_tuple(st) == g.state()
                assert st.misses == 0 and st.balls == 0 and st.ball_y == 32
                ret, length, episodes = 0.0, 0, episodes + 1
            else:
                assert cnt == 1
        assert episodes >= 1500 // hi - 1


def _args(argv):
    import train
    return train.get_arg_parser().parse_args(argv)


def test_shard_equals_union():
    """Envs [0, 8) of one creator == envs [0, 4) of a creator at offset 0 and of one at offset 4."""
    from manette_amd.environment_creator import EnvironmentCreator
    union = _args(['-g', 'catch', '--seed', '5'])
    hi = _args(['-g', 'catch', '--seed', '5'])
    hi.env_id_offset = 4
    cu, ch = EnvironmentCreator(union), EnvironmentCreator(hi)
    whole = [cu.create_environment(i) for i in range(8)]
    parts = [cu.create_environment(i) for i in range(4)] + [ch.create_environment(i) for i in range(4)]
    for i, (x, y) in enumerate(zip(whole, parts)):
        np.testing.assert_array_equal(x.get_initial_state(), y.get_initial_state())
        for step in range(40):
            a, _ = catch_ref.hashed_actions(step, i, 1)
            ox, rx, dx = x.next(a)
            oy, ry, dy = y.next(a)
            assert (rx, dx) == (ry, dy)
            np.testing.assert_array_equal(ox, oy)
    # and the envs differ from one another (the ball stream hashes the global env id)
    assert len({_state_tuple(e.state) for e in whole}) > 1


def _tracker(st):
    """Keep the paddle's middle under the ball's: the action whose paddle, 4 sub-frames on, is nearest."""
    bx = min(80, max(0, st.ball_x + 4 * st.ball_dx))
    best = None
    for a, d in ((0, 0), (1, -8), (2, 8)):
        px = min(72, max(0, st.paddle_x + d))
        key = abs(bx - 4 - px)
        if best is None or key < best[0]:
            best = (key, a)
    return best[1]


def _play(cfg, env, policy, episodes):
    st = _lib.mt_catch_state()
    catch.host_reset(cfg, SEED, env, 1, st)
    out, ret, catches = [], 0.0, 0
    while len(out) < episodes:
        rw, over, _ = catch.host_step(cfg, SEED, env, 1, TAB1, policy(st), 0, st)
        ret += rw
        catches += rw > 0
        if over:
            out.append((ret, catches))
            ret, catches = 0.0, 0
    return out


def test_game_is_controllable():
    """A paddle that tracks the ball catches every ball (return = max_balls); a noop paddle loses its
    lives (return = its catches - lives). So max_balls, the top of the learning bar, is attainable."""
    cfg = catch.config(3, 20)
    for ret, catches in _play(cfg, 7, _tracker, 50):
        assert (ret, catches) == (20.0, 20)
    for ret, catches in _play(cfg, 7, lambda st: 0, 50):
        assert ret == catches - 3 and ret < 20


@pytest.mark.parametrize('lives,max_balls', [(1, 2), (3, 20)])
def test_runner_contract(lives, max_balls):
    """CatchEmulator under the reference-contract runner loop == mt_catch_step_host driven directly."""
    from manette_amd.emulator_runner import run_emulators
    E = 3
    cfg = catch.config(lives, max_balls)
    emus = [catch.CatchEmulator(10 + e, seed=SEED, lives=lives, max_balls=max_balls) for e in range(E)]
    states = np.asarray([e.get_initial_state() for e in emus])
    variables = [states, np.zeros(E, np.float32), np.zeros(E, np.float32), np.zeros(E, np.int32), np.zeros(E, np.int32)]
    sts = [_lib.mt_catch_state() for _ in range(E)]
    obs = [np.zeros((84, 84, 4), np.uint8) for _ in range(E)]
    for e in range(E):
        catch.host_reset(cfg, SEED, 10 + e, 1, sts[e], obs[e])
        np.testing.assert_array_equal(states[e], obs[e])
    for step in range(80):
        for e in range(E):
            variables[3][e], variables[4][e] = catch_ref.hashed_actions(step, e, 11)
        run_emulators(list(TAB11), emus, variables)
        for e in range(E):
            out = np.empty_like(obs[e])
            rw, over, _ = catch.host_step(cfg, SEED, 10 + e, 1, TAB11, variables[3][e], variables[4][e], sts[e],
                                          obs[e], out)
            obs[e] = out
            assert (variables[1][e], bool(variables[2][e])) == (rw, over), (step, e)
            np.testing.assert_array_equal(variables[0][e], out)
            assert _state_tuple(emus[e].state) == _state_tuple(sts[e])


def test_argument_checks():
    import train
    from manette_amd.environment_creator import EnvironmentCreator
    from manette_amd.paac import check_arch_flags
    assert EnvironmentCreator(_args(['-g', 'catch'])).num_actions == 3
    train.validate_args(_args(['-g', 'catch', '--runner', 'device', '--arch', 'NIPS']))
    train.validate_args(_args(['-g', 'catch', '--runner', 'python', '--arch', 'LSTM']))
    with pytest.raises(ValueError, match='device environment'):
        train.validate_args(_args(['-g', 'pong', '--runner', 'device', '--arch', 'NIPS']))
    with pytest.raises(ValueError, match='LSTM'):
        check_arch_flags(_args(['-g', 'catch', '--runner', 'device', '--arch', 'LSTM']))
    with pytest.raises(ValueError, match='device environment'):
        EnvironmentCreator(_args(['-g', 'pong'])).create_device_env(4, [0])
    # the C ABI's own checks: before anything runs
    lib = _lib.hip()
    st = _lib.mt_catch_state()
    rw, ov = C.c_float(), C.c_float()
    tab = TAB1.ctypes.data_as(C.c_void_p)
    for cfg, depth in ((catch.config(0, 20), 1), (catch.config(3, 0), 1), (catch.config(3, 20), 2)):
        assert lib.mt_catch_reset_host(C.byref(cfg), 0, 0, depth, C.byref(st), None) == 1
        assert lib.mt_catch_step_host(C.byref(cfg), 0, 0, depth, tab, 1, 0, 0, C.byref(st), None, None, None, None,
                                      C.byref(rw), C.byref(ov)) == 1
    ok = catch.config(3, 20)
    for args in ((C.byref(ok), 0, 0, 0, 1, None, None, None), (C.byref(ok), 0, -1, 4, 1, None, None, None),
                 (C.byref(ok), 0, 0, 4, 2, None, None, None), (None, 0, 0, 4, 1, None, None, None)):
        assert lib.mt_catch_reset(*args) == 1  # (refused before any launch: no GPU is touched)
    assert lib.mt_catch_step(C.byref(ok), 0, 0, 4, 1, None, 1, None, None, None, None, None, None, None, None, None,
                             None, 0, 5, None) == 1


def test_out_of_range_indices_are_clamped():
    cfg = catch.config(3, 20)
    for (a, r), (ac, rc) in (((-5, -1), (0, 0)), ((9, 99), (2, 10)), ((1, 3), (1, 3))):
        s1, s2 = _lib.mt_catch_state(), _lib.mt_catch_state()
        catch.host_reset(cfg, SEED, 1, 1, s1)
        catch.host_reset(cfg, SEED, 1, 1, s2)
        assert catch.host_step(cfg, SEED, 1, 1, TAB11, a, r, s1) == catch.host_step(cfg, SEED, 1, 1, TAB11, ac, rc, s2)
        assert _state_tuple(s1) == _state_tuple(s2)
        assert catch_ref.clamp_indices(a, r, 11) == (ac, rc)
