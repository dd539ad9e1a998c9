"""Tetris: the reference's own game (tetris.py / tetris_emulator.py, `-g tetris`: a 10 x 22 board of coloured
cells, seven pieces with four rotations, row removal, levels, five actions), its rule restated in
include/manette_hip.h ("Tetris") and pinned act by act to recordings of the reference's code. Its
description, and its two faces (manette_amd/device_game.py) under the game's own names: TetrisEmulator on
the host restatement, TetrisDevice in HBM. Both key an env's piece draws on (seed, global env id), so they
play the same games.
"""
from . import device_game

NUM_ACTIONS = 5
DEFAULT_MAX_NEXTS = 2000
DEFAULT_SPEED = 5
DEFAULT_MAX_START_WAIT = 0
RANDOM_START_WAIT = 30  # tetris_emulator.py's MAX_START_WAIT, under --random_start


def max_episode_nexts(cfg):
    """An upper bound on the next() calls of one episode (so on its macro-steps, each of which plays at
    least one): the rule ends an episode when nexts >= max_nexts."""
    return int(cfg.max_nexts)


def _from_args(args):
    """max_start_wait has no flag of its own: --random_start asks for the reference's 30."""
    return {'max_start_wait': RANDOM_START_WAIT if getattr(args, 'random_start', False) else DEFAULT_MAX_START_WAIT}


GAME = device_game.Game('tetris', NUM_ACTIONS, [('max_nexts', DEFAULT_MAX_NEXTS), ('speed', DEFAULT_SPEED),
                                                ('max_start_wait', DEFAULT_MAX_START_WAIT)], max_episode_nexts,
                        from_args=_from_args, reference=True)
STATE_BYTES, STATE_DTYPE = GAME.state_bytes, GAME.state_dtype
assert STATE_DTYPE.itemsize == STATE_BYTES == 136
config, host_reset, host_step = GAME.config, GAME.host_reset, GAME.host_step
TetrisEmulator, TetrisDevice = GAME.Emulator, GAME.Device
