"""Catch: a small real game (a paddle, falling balls, lives, three actions) whose rule is written out
in include/manette_hip.h ("Catch"). Its description, and its two faces (manette_amd/device_game.py) under
the game's own names: CatchEmulator on the host restatement, CatchDevice in HBM. Both key an env's ball
stream on (seed, global env id), so they play the same games.
"""
from . import device_game

NUM_ACTIONS = 3
DEFAULT_LIVES = 3
DEFAULT_MAX_BALLS = 20


def max_episode_nexts(cfg):
    """An upper bound on the next() calls of one episode (so on its macro-steps, each of which plays at
    least one): an episode sees at most max_balls balls, a ball needs 38 sub-frames from its spawn to
    the paddle row (the rule, "next(a)") and the following ball spawns in the sub-frame that settled the
    last, so an episode has at most 38 * max_balls sub-frames, four to a next."""
    return (38 * int(cfg.max_balls) + 3) // 4


GAME = device_game.Game('catch', NUM_ACTIONS, [('lives', DEFAULT_LIVES), ('max_balls', DEFAULT_MAX_BALLS)],
                        max_episode_nexts)
STATE_BYTES, STATE_DTYPE = GAME.state_bytes, GAME.state_dtype
assert STATE_DTYPE.itemsize == STATE_BYTES == 32
config, host_reset, host_step = GAME.config, GAME.host_reset, GAME.host_step
CatchEmulator, CatchDevice = GAME.Emulator, GAME.Device
