"""Tetris on the host (no GPU): mt_tetris_step_host against recordings of the reference's own TetrisApp
(tests/golden/tetris_rule.npz: played episodes and crafted single acts, field for field at every act), the
host render against a numpy restatement, episode bounds, the piece carried over a game end, the start wait,
argument refusals, the emulator face, and that the game is controllable."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

import tetris_cases
import tetris_ref
from manette_amd import _lib, tetris

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tetris_rule.npz')
ONE = np.zeros(1, np.int32)
UNCAPPED = 1 << 30
STATE_KEYS = ('x', 'y', 'next_piece', 'level', 'lines', 'speed', 'speed_counter', 'piece_counter')


@pytest.fixture(scope='module')
def gold():
    g = dict(np.load(GOLDEN))
    _assert_coverage(g)  # a thin fixture cannot pass: checked before any test uses it
    return g


def _traces(g):
    s = g['trace_start']
    return [(str(g['trace_name'][k]), int(g['trace_seed'][k]), int(g['trace_env'][k]), int(s[k]), int(s[k + 1]))
            for k in range(len(s) - 1)]


def _assert_coverage(g):
    """The played episodes alone: >= 1 single-row and >= 1 multi-row clear, >= 2 level-ups, >= 3 game overs,
    >= 1 refused rotation, >= 1 refused move; all three policies; the crafted cases are tetris_cases.py's."""
    single = multi = levelups = overs = refused_rot = refused_move = 0
    for _, _, _, lo, hi in _traces(g):
        for i in range(lo + 1, hi):
            if g['t_init'][i] or g['t_init'][i - 1] or g['t_gameover'][i - 1]:
                continue  # (a new game's acts; the act before was another game's)
            dl = int(g['t_lines'][i]) - int(g['t_lines'][i - 1])
            single += dl == 1
            multi += dl > 1
            levelups += int(g['t_level'][i]) > int(g['t_level'][i - 1])
            same_piece = g['t_piece_counter'][i] == g['t_piece_counter'][i - 1]
            a = int(g['t_action'][i])
            if a == 4 and same_piece and g['t_stone_w'][i] != g['t_stone_h'][i]:  # (not the square)
                refused_rot += np.array_equal(g['t_stone'][i], g['t_stone'][i - 1])
            if a in (1, 2) and same_piece:
                w, x0 = int(g['t_stone_w'][i]), int(g['t_x'][i - 1])
                inside = 0 <= x0 + (-1 if a == 1 else 1) <= 10 - w
                refused_move += inside and int(g['t_x'][i]) == x0
        overs += int(g['t_gameover'][lo:hi].sum())
    assert single >= 1 and multi >= 1 and levelups >= 2 and overs >= 3 and refused_rot >= 1 and refused_move >= 1, \
        (single, multi, levelups, overs, refused_rot, refused_move)
    assert set(g['trace_name'].tolist()) == {'random', 'drop', 'scripted'}
    assert g['case_name'].tolist() == [c[0] for c in tetris_cases.CASES]
    for k, (_, s, a) in enumerate(tetris_cases.CASES):
        np.testing.assert_array_equal(g['casepre_board'][k], np.asarray(s['board'], np.uint8))
        assert (int(g['casepre_x'][k]), int(g['casepre_y'][k]), int(g['case_action'][k])) == (s['x'], s['y'], a)
    names = set(g['case_name'].tolist())
    assert {'clear_1', 'clear_2', 'clear_3', 'clear_4', 'clear_levels_up', 'level_up_speed_already_1',
            'over_on_spawn_with_full_row', 'drop_locks_then_gravity', 'rotate_refused_right_wall',
            'rotate_refused_by_stack', 'move_left_clamped', 'move_left_refused', 'gravity_only_lock'} <= names
    assert os.path.getsize(GOLDEN) <= 300 * 1024


def test_fixture_covers_the_rule(gold):
    _assert_coverage(gold)


def _assert_fields(st, g, prefix, i, where):
    np.testing.assert_array_equal(tetris_ref.words_board(list(st.board)), g[prefix + 'board'][i], err_msg='board ' + where)
    h, w = int(g[prefix + 'stone_h'][i]), int(g[prefix + 'stone_w'][i])
    assert tetris_ref.matrix(st.piece, st.rot) == g[prefix + 'stone'][i][:h, :w].tolist(), 'piece ' + where
    for k in STATE_KEYS:
        assert int(getattr(st, k)) == int(g[prefix + k][i]), '%s %s' % (k, where)


def test_rule_matches_the_reference_traces(gold):
    """Every recorded act of every trace: reward, game over and, field for field, the state after it (after a
    game over: the state after the new game's four initial acts)."""
    g = gold
    cfg = tetris.config(UNCAPPED, 5, 0)
    acts = 0
    for name, seed, env, lo, hi in _traces(g):
        st = _lib.mt_tetris_state()
        tetris.host_reset(cfg, seed, env, 1, st)
        assert g['t_init'][lo:lo + 4].all()
        _assert_fields(st, g, 't_', lo + 3, '%s reset' % name)
        i = lo + 4
        while i < hi:
            assert not g['t_init'][i]
            rw, over, _ = tetris.host_step(cfg, seed, env, 1, ONE, int(g['t_action'][i]), 0, st)
            where = '%s act %d' % (name, i - lo)
            assert rw == float(g['t_reward'][i]) and over == bool(g['t_gameover'][i]), where
            acts += 1
            if over:
                assert g['t_init'][i + 1:i + 5].all()
                i += 4
                assert st.nexts == 0
            _assert_fields(st, g, 't_', i, where)
            i += 1
    assert acts > 4000


def test_rule_matches_the_reference_on_crafted_acts(gold):
    g = gold
    cfg = tetris.config(UNCAPPED, 5, 0)
    for k, (name, s, a) in enumerate(tetris_cases.CASES):
        st = tetris_ref.fill_state(_lib.mt_tetris_state(), **s)
        rw, over, _ = tetris.host_step(cfg, tetris_cases.SEED, tetris_cases.ENV, 1, ONE, a, 0, st)
        assert rw == float(g['case_reward'][k]) and over == bool(g['case_gameover'][k]), name
        if not over:
            _assert_fields(st, g, 'case_', k, name)
            assert st.nexts == s['nexts'] + 1
    assert g['case_gameover'].sum() >= 1


# ---- render ------------------------------------------------------------------------------------------
def _render_samples():
    stack_rows = {y: '1234567012' for y in range(14, 22)}
    stack_rows[13] = '0070000400'
    out = []
    for piece in range(1, 8):
        for rot in range(4):
            w = len(tetris_ref.matrix(piece, rot)[0])
            h = len(tetris_ref.matrix(piece, rot))
            out.append(tetris_cases.st({}, piece, rot, 0, 0, next_piece=1 + (piece + rot) % 7))  # left wall, top
            out.append(tetris_cases.st(stack_rows, piece, rot, 10 - w, 13 - h, next_piece=piece))  # right wall, box
            out.append(tetris_cases.st(stack_rows, piece, rot, 4, 12 - h, next_piece=1 + (piece * 3) % 7))  # over it
    out.append(tetris_cases.st({}, 6, 1, 9, 18))  # the floor
    return out


@pytest.mark.parametrize('depth', [1, 3])
def test_host_render_equals_numpy(depth):
    """A noop act without gravity leaves the state as it is: its frame is the state's render. Every piece at
    every rotation, at both walls, over a stack and beside the next-piece box; the stacked state too."""
    cfg = tetris.config(UNCAPPED, 5, 0)
    rs = np.random.RandomState(depth)
    for k, s in enumerate(_render_samples()):
        st = tetris_ref.fill_state(_lib.mt_tetris_state(), **s)
        prev = rs.randint(0, 256, (84, 84, 4 * depth)).astype(np.uint8)
        out, frames = np.zeros_like(prev), np.zeros((4, 84, 84, depth), np.uint8)
        rw, over, cnt = tetris.host_step(cfg, 1, 0, depth, ONE, 0, 0, st, prev, out, frames)
        assert (rw, over, cnt) == (0.0, False, 1) and st.y == s['y']
        want = tetris_ref.render(np.asarray(s['board']), s['piece'], s['rot'], s['x'], s['y'], s['next_piece'], depth)
        np.testing.assert_array_equal(frames[0], want, err_msg='sample %d' % k)
        np.testing.assert_array_equal(out, tetris_ref.stack(prev, [want], depth), err_msg='stack, sample %d' % k)


def test_render_geometry_and_colours():
    """No sampled column is the separator line's (source x = 181); every cell row and column of the screen is
    sampled; the gray table is pairwise distinct."""
    xs = [((2 * j + 1) * 12) // 7 for j in range(84)]
    assert 181 not in xs and max(xs) < 288
    assert sorted(set(tetris_ref.sample_cols())) == list(range(16))
    assert sorted(set(tetris_ref.sample_rows())) == list(range(22))
    assert len(set(tetris_ref.GRAY)) == 9 and len(set(tetris_ref.RGB)) == 9


def test_multi_push_stack_and_frames():
    """R = 11: more than four nexts in a macro-step keep the last four frames, each the render of its own state
    (checked by replaying the same nexts one at a time)."""
    cfg = tetris.config(UNCAPPED, 2, 0)
    tab = np.arange(11, dtype=np.int32)
    a_st, b_st = _lib.mt_tetris_state(), _lib.mt_tetris_state()
    obs = np.zeros((84, 84, 4), np.uint8)
    tetris.host_reset(cfg, 5, 2, 1, a_st, obs)
    tetris.host_reset(cfg, 5, 2, 1, b_st)
    np.testing.assert_array_equal(obs[..., 3], tetris_ref.render_state(a_st, 1)[..., 0])
    for step, (a, r) in enumerate([(3, 6), (1, 2), (4, 0), (3, 10)]):
        out, frames = np.zeros_like(obs), np.zeros((4, 84, 84, 1), np.uint8)
        rw, over, cnt = tetris.host_step(cfg, 5, 2, 1, tab, a, r, a_st, obs, out, frames)
        singles, total = [], 0.0
        for _ in range(r + 1):
            rw1, ov1, _ = tetris.host_step(cfg, 5, 2, 1, ONE, a, 0, b_st)
            singles.append(tetris_ref.render_state(b_st, 1))
            total += rw1
            assert not ov1
        assert (rw, over, cnt) == (total, False, min(4, r + 1))
        for j, f in enumerate(singles[-4:]):
            np.testing.assert_array_equal(frames[j], f, err_msg='step %d frame %d' % (step, j))
        np.testing.assert_array_equal(out, tetris_ref.stack(obs, singles, 1))
        assert bytes(a_st) == bytes(b_st)
        obs = out


# ---- episodes ----------------------------------------------------------------------------------------
def test_max_nexts_ends_an_episode_and_the_next_piece_carries_over():
    cfg = tetris.config(7, 5, 0)
    assert tetris.max_episode_nexts(cfg) == 7
    st = _lib.mt_tetris_state()
    tetris.host_reset(cfg, 11, 4, 1, st)
    for episode in range(3):
        for k in range(7):
            assert st.nexts == k
            nxt, counter = st.next_piece, st.piece_counter
            rw, over, cnt = tetris.host_step(cfg, 11, 4, 1, ONE, 0, 0, st)
            assert over == (k == 6) and rw == 0.0
        # the new game: its piece is the old game's next piece, its next piece the stream's next draw
        assert st.piece == nxt and st.piece_counter == counter + 1 and cnt == 4
        assert st.next_piece == 1 + tetris_ref.piece_draw(11, 4, counter)
        assert (st.level, st.lines, st.speed, st.speed_counter, st.nexts) == (1, 0, 5, 4, 0)
        assert not any(st.board)
    tab = np.asarray([10], np.int32)  # a macro-step stops at the episode end
    rw, over, cnt = tetris.host_step(cfg, 11, 4, 1, tab, 3, 0, st)
    assert over and rw == 7.0 and st.nexts == 0


@pytest.mark.parametrize('depth', [1, 3])
def test_start_wait(depth):
    """max_start_wait 30: a new game plays w noop acts (w from the draw stream under the wait salt) before the
    four whose frames are the initial state: the same state and stack as w more noops after a wait-0 reset.
    max_start_wait 0: four acts, the last frame the state's render."""
    c0, c30 = tetris.config(UNCAPPED, 5, 0), tetris.config(UNCAPPED, 5, 30)
    waits = set()
    for env in range(6):
        a, b = _lib.mt_tetris_state(), _lib.mt_tetris_state()
        oa, ob = np.zeros((84, 84, 4 * depth), np.uint8), np.zeros((84, 84, 4 * depth), np.uint8)
        tetris.host_reset(c30, 99, env, depth, a, oa)
        tetris.host_reset(c0, 99, env, depth, b, ob)
        assert b.speed_counter == 4 and b.y == 1 and b.nexts == 0
        np.testing.assert_array_equal(ob.reshape(84, 84, depth, 4)[..., 3], tetris_ref.render_state(b, depth))
        w = tetris_ref.start_wait(99, env, 2, 30)  # (two pieces drawn: piece_counter = 2)
        waits.add(w)
        for _ in range(w):
            nb = np.zeros_like(ob)
            tetris.host_step(c0, 99, env, depth, ONE, 0, 0, b, ob, nb)
            ob = nb
        assert a.speed_counter == w + 4 and a.nexts == 0
        b.nexts = 0
        assert bytes(a) == bytes(b)
        np.testing.assert_array_equal(oa, ob)
    assert len(waits) > 2 and max(waits) <= 30


def test_host_argument_refusals():
    lib = _lib.hip()
    st = _lib.mt_tetris_state()
    good = tetris.config()
    tetris.host_reset(good, 0, 0, 1, st)
    buf, buf2 = np.zeros((84, 84, 4), np.uint8), np.zeros((84, 84, 4), np.uint8)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    rw, ov, cnt = C.c_float(), C.c_float(), C.c_int32()
    before = bytes(st)

    def step(cfg=good, depth=1, tab=ONE, R=1, state=st, prev=None, out=None):
        return lib.mt_tetris_step_host(C.byref(cfg) if cfg is not None else None, C.c_uint64(0), C.c_uint64(0), depth,
                                       p(tab) if tab is not None else None, R, 0, 0,
                                       C.byref(state) if state is not None else None, prev, out, None, C.byref(cnt),
                                       C.byref(rw), C.byref(ov))

    for kw in (dict(cfg=tetris.config(0, 5, 0)), dict(cfg=tetris.config(10, 0, 0)), dict(cfg=tetris.config(10, 5, -1)),
               dict(cfg=tetris.config(10, 5, 31)), dict(cfg=None), dict(depth=2), dict(tab=None), dict(R=0),
               dict(state=None), dict(out=p(buf)), dict(prev=p(buf), out=p(buf))):
        assert step(**kw) == 1, kw
    assert bytes(st) == before
    assert step(prev=p(buf), out=p(buf2)) == 0
    assert lib.mt_tetris_reset_host(C.byref(good), C.c_uint64(0), C.c_uint64(0), 1, None, None) == 1
    assert lib.mt_tetris_reset_host(C.byref(good), C.c_uint64(0), C.c_uint64(0), 4, C.byref(st), None) == 1
    assert lib.mt_tetris_reset_host(C.byref(tetris.config(1, 1, 31)), C.c_uint64(0), C.c_uint64(0), 1, C.byref(st), None) == 1


def test_wild_state_and_indices_are_clamped():
    """A state of garbage and out-of-range indices play without reading outside the board."""
    cfg = tetris.config(50, 1, 0)
    rs = np.random.RandomState(7)
    tab = np.asarray([0, 300, -5], np.int32)
    for _ in range(20):
        raw = rs.randint(0, 256, tetris.STATE_BYTES).astype(np.uint8)
        st = _lib.mt_tetris_state.from_buffer_copy(raw.tobytes())
        for a, r in ((-9, -9), (77, 1), (4, 2)):
            tetris.host_step(cfg, 1, 2, 1, tab, a, r, st)
            assert 1 <= st.piece <= 7 and 0 <= st.rot <= 3 and 0 <= st.x <= 9 and 0 <= st.y <= 21
            assert all(w < (1 << 30) for w in st.board)


# ---- the emulator face -------------------------------------------------------------------------------
def test_emulator_through_environment_creator():
    from manette_amd.environment_creator import ALL_DEVICE_GAMES, EnvironmentCreator, has_device_env
    assert 'tetris' in ALL_DEVICE_GAMES and has_device_env('tetris')
    args = argparse.Namespace(game='tetris', rgb=False, seed=3, tetris_max_nexts=9, tetris_speed=5, random_start=False)
    ec = EnvironmentCreator(args)
    assert ec.num_actions == 5 == tetris.NUM_ACTIONS
    em = ec.create_environment(2)
    assert isinstance(em, tetris.TetrisEmulator) and list(em.get_legal_actions()) == [0, 1, 2, 3, 4]
    s0 = em.get_initial_state()
    assert s0.shape == (84, 84, 4) and s0.dtype == np.uint8 and em.cfg.max_start_wait == 0
    total = 0
    for k in range(9):
        s, rw, over = em.next(3)
        total += rw
        assert over == (k == 8) and rw == 1.0
    np.testing.assert_array_equal(em.get_initial_state(), s)  # the new game's state, not played again
    rgb = EnvironmentCreator(argparse.Namespace(game='tetris', rgb=True, seed=3, random_start=True))
    e2 = rgb.create_environment(0)
    assert e2.get_initial_state().shape == (84, 84, 12) and e2.cfg.max_start_wait == 30 and e2.cfg.max_nexts == 2000
    for name in ('tetris-v0', 'Catcher-v0'):
        with pytest.raises(NotImplementedError):
            EnvironmentCreator(argparse.Namespace(game=name))
    with pytest.raises(ValueError):
        ec.create_bank(0, 2)


def _episode_returns(cfg, seed, env, choose, episodes):
    st = _lib.mt_tetris_state()
    tetris.host_reset(cfg, seed, env, 1, st)
    rets, ret = [], 0.0
    while len(rets) < episodes:
        rw, over, _ = tetris.host_step(cfg, seed, env, 1, ONE, choose(st), 0, st)
        ret += rw
        if over:
            rets.append(ret)
            ret = 0.0
    return rets


def test_game_is_controllable():
    """A scripted placement policy on the host face scores >= 10 x the uniform-random policy's mean return, 20
    episodes each at the default config."""
    cfg = tetris.config()
    rs = np.random.RandomState(12345)
    random_mean = float(np.mean(_episode_returns(cfg, 0, 0, lambda st: int(rs.randint(5)), 20)))
    placer = tetris_ref.PlacementPolicy()
    scripted = _episode_returns(
        cfg, 0, 1, lambda st: placer.action(st.piece_counter, tetris_ref.words_board(list(st.board)),
                                            st.piece, st.rot, st.x, st.y), 20)
    print('random %.1f  scripted mean %.1f min %.1f' % (random_mean, np.mean(scripted), np.min(scripted)))
    assert random_mean > 0 and np.mean(scripted) >= 10.0 * random_mean
