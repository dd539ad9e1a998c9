"""Bricks: a Breakout-like real game (a paddle, a ball, a wall of 6 x 14 bricks, lives, four actions)
whose rule is written out in include/manette_hip.h ("Bricks"). Its description, and its two faces
(manette_amd/device_game.py) under the game's own names: BricksEmulator on the host restatement,
BricksDevice in HBM. Both key an env's serves on (seed, global env id), so they play the same games.
"""
from . import device_game

NUM_ACTIONS = 4
DEFAULT_LIVES = 3
DEFAULT_MAX_NEXTS = 500
DEFAULT_SERVE_WAIT = 4


def max_episode_nexts(cfg):
    """An upper bound on the next() calls of one episode (so on its macro-steps, each of which plays at
    least one): the rule ends an episode when nexts >= max_nexts."""
    return int(cfg.max_nexts)


GAME = device_game.Game('bricks', NUM_ACTIONS, [('lives', DEFAULT_LIVES), ('max_nexts', DEFAULT_MAX_NEXTS),
                                                ('serve_wait', DEFAULT_SERVE_WAIT)], max_episode_nexts)
STATE_BYTES, STATE_DTYPE = GAME.state_bytes, GAME.state_dtype
assert STATE_DTYPE.itemsize == STATE_BYTES == 56
config, host_reset, host_step = GAME.config, GAME.host_reset, GAME.host_step
BricksEmulator, BricksDevice = GAME.Emulator, GAME.Device
