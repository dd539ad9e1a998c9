"""The contract the device games share (no GPU): every game of ALL_DEVICE_GAMES has a complete description,
a refusal names the entry point that made it, the clamps of the action and repetition indices are the
game's own, and the emulator of a game plays what its host face plays."""
import ctypes as C
import importlib

import numpy as np
import pytest

from manette_amd import _lib
from manette_amd.environment_creator import ALL_DEVICE_GAMES, EnvironmentCreator

SEED = 0x1234567
TAB11 = np.arange(11, dtype=np.int32)
# a config the game's own check refuses
BAD_CONFIG = {'catch': (0, 20), 'bricks': (0, 500, 4), 'tetris': (0, 5, 0)}


def _module(game):
    return importlib.import_module('manette_amd.' + game)


def _state_class(game):
    return getattr(_lib, 'mt_%s_state' % game)


def _args(argv):
    import train
    return train.get_arg_parser().parse_args(argv)


def test_every_device_game_is_covered():
    assert set(BAD_CONFIG) == set(ALL_DEVICE_GAMES)


def test_registry_describes_every_game():
    """The registry (manette_amd/device_game.py) is where the game lists come from, and a game's module
    re-exports what its description holds."""
    from manette_amd import device_game, environment_creator as ec
    reg = device_game.games()
    assert tuple(reg) == ALL_DEVICE_GAMES == ec.DEVICE_GAMES + ec.REFERENCE_DEVICE_GAMES
    assert ec.REFERENCE_DEVICE_GAMES == tuple(n for n in reg if reg[n].reference) == ('tetris',)
    for name, g in reg.items():
        mod = _module(name)
        assert g is mod.GAME and g.name == name and g.num_actions == mod.NUM_ACTIONS
        assert sorted(g.symbols.values()) == sorted('mt_%s_%s' % (name, fn)
                                                    for fn in ('reset', 'step', 'reset_host', 'step_host'))
        assert (g.state_bytes, g.state_dtype, g.state_class) == (mod.STATE_BYTES, mod.STATE_DTYPE, _state_class(name))
        assert g.Emulator is getattr(mod, name.capitalize() + 'Emulator')
        assert g.Device is getattr(mod, name.capitalize() + 'Device')
        emu = g.Emulator(0)
        assert bytes(emu.cfg) == bytes(mod.config()) and emu.max_episode_nexts() == mod.max_episode_nexts(emu.cfg)


@pytest.mark.parametrize('game', ALL_DEVICE_GAMES)
def test_description_is_complete(game):
    mod, lib = _module(game), _lib.hip()
    for fn in ('reset', 'step', 'reset_host', 'step_host'):
        assert callable(getattr(lib, 'mt_%s_%s' % (game, fn)))
    assert mod.STATE_DTYPE.itemsize == mod.STATE_BYTES == C.sizeof(_state_class(game))
    assert isinstance(mod.config(), getattr(_lib, 'mt_%s_config' % game))
    assert mod.max_episode_nexts(mod.config()) >= 1
    ec = EnvironmentCreator(_args(['-g', game]))
    assert ec.num_actions == mod.NUM_ACTIONS
    emu = ec.create_environment(0)
    assert isinstance(emu, getattr(mod, game.capitalize() + 'Emulator'))
    assert list(emu.get_legal_actions()) == list(range(mod.NUM_ACTIONS))
    assert hasattr(mod, game.capitalize() + 'Device')


@pytest.mark.parametrize('game', ALL_DEVICE_GAMES)
def test_refusals_name_their_entry_point(game):
    """Every refusal below comes before any launch (no GPU is touched): status 1, and a message that starts
    with the public name of the entry point that was called."""
    mod, lib = _module(game), _lib.hip()
    fn = {k: getattr(lib, 'mt_%s_%s' % (game, k)) for k in ('reset', 'step', 'reset_host', 'step_host')}
    st = _state_class(game)()
    rw, ov = C.c_float(), C.c_float()
    tab = TAB11.ctypes.data_as(C.c_void_p)
    obs = np.zeros((84, 84, 4), np.uint8)
    p = obs.ctypes.data_as(C.c_void_p)
    ok, bad = mod.config(), mod.config(*BAD_CONFIG[game])
    calls = []
    for cfg, depth in ((bad, 1), (ok, 2), (None, 1)):
        ref = None if cfg is None else C.byref(cfg)
        calls += [('reset_host', (ref, 0, 0, depth, C.byref(st), None)),
                  ('step_host', (ref, 0, 0, depth, tab, 1, 0, 0, C.byref(st), None, None, None, None, C.byref(rw),
                                 C.byref(ov))),
                  ('reset', (ref, 0, 0, 4, depth, None, None, None)),
                  ('step', (ref, 0, 0, 4, depth, None, 1, None, None, None, None, None, None, None, None, None, None,
                            0, 5, None))]
    calls += [('reset_host', (C.byref(ok), 0, 0, 1, None, None)),  # null state
              ('step_host', (C.byref(ok), 0, 0, 1, tab, 0, 0, 0, C.byref(st), None, None, None, None, C.byref(rw),
                             C.byref(ov))),  # R < 1
              ('step_host', (C.byref(ok), 0, 0, 1, tab, 1, 0, 0, C.byref(st), p, p, None, None, C.byref(rw),
                             C.byref(ov))),  # out aliases prev
              ('reset', (C.byref(ok), 0, 0, 0, 1, None, None, None)),   # E < 1
              ('reset', (C.byref(ok), 0, -1, 4, 1, None, None, None)),  # env0 < 0
              ('reset', (C.byref(ok), 0, 0, 4, 1, None, None, None)),   # null buffers
              ('step', (C.byref(ok), 0, 0, 4, 1, None, 0, None, None, None, None, None, None, None, None, None, None,
                        0, 5, None)),   # R < 1
              ('step', (C.byref(ok), 0, 0, 4, 1, None, 1, None, None, None, None, None, None, None, None, None, None,
                        5, 5, None)),   # t outside [0, T)
              ('step', (C.byref(ok), 0, 0, 4, 1, None, 1, None, None, None, None, None, None, None, None, None, None,
                        0, 5, None))]   # null buffers
    assert {k for k, _ in calls} == set(fn)
    for k, args in calls:
        assert fn[k](*args) == 1, (k, args)
        msg = lib.mt_last_error().decode()
        assert msg.startswith('mt_%s_%s: ' % (game, k)), (k, msg)


def _play(mod, game, steps):
    """Two macro-steps from a reset on the host face under (a, r) pairs: everything the face returns."""
    cfg = mod.config()
    st = _state_class(game)()
    obs = np.zeros((84, 84, 4), np.uint8)
    mod.host_reset(cfg, SEED, 3, 1, st, obs)
    got = []
    for a, r in steps:
        out = np.empty_like(obs)
        got.append(mod.host_step(cfg, SEED, 3, 1, TAB11, a, r, st, obs, out))
        obs = out
    return got, bytes(st), obs


@pytest.mark.parametrize('game', ALL_DEVICE_GAMES)
def test_clamps_are_per_game(game):
    mod = _module(game)
    top = mod.NUM_ACTIONS - 1
    for (a, r), (ac, rc) in (((99, 2), (top, 2)), ((-5, 2), (0, 2)), ((1, 99), (1, 10)), ((1, -5), (1, 0)),
                             ((99, 99), (top, 10))):
        got, st, obs = _play(mod, game, [(a, r)] * 2)
        want, st_c, obs_c = _play(mod, game, [(ac, rc)] * 2)
        assert got == want and st == st_c, (a, r)
        np.testing.assert_array_equal(obs, obs_c)
    # the top action is the game's own: one below it plays another game within two macro-steps of 11 nexts
    assert _play(mod, game, [(top, 10)] * 2)[1:2] != _play(mod, game, [(top - 1, 10)] * 2)[1:2]


@pytest.mark.parametrize('game', ALL_DEVICE_GAMES)
@pytest.mark.parametrize('rgb', [False, True])
def test_faces_play_the_same_game(game, rgb):
    mod = _module(game)
    argv = ['-g', game, '--seed', '5'] + (['--rgb'] if rgb else [])
    ec = EnvironmentCreator(_args(argv))
    depth = 3 if rgb else 1
    for i in (0, 2):
        emu = ec.create_environment(i)
        st = _state_class(game)()
        obs = np.zeros((84, 84, 4 * depth), np.uint8)
        mod.host_reset(emu.cfg, 5, i, depth, st, obs)
        np.testing.assert_array_equal(emu.get_initial_state(), obs)
        assert bytes(emu.state) == bytes(st)
