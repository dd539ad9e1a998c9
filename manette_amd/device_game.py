"""The device games' shared layer: what a game is (Game, its description) and the two faces every game
has, written once (include/manette_hip.h: "Catch", "Bricks", "Tetris"; csrc/device_game.h is the C++ side).

  * Emulator: the reference contract (BaseEnvironment) on the host restatement of the rule
    (mt_<game>_reset_host / mt_<game>_step_host, no GPU needed) — the Python runner, test.py, CPU paths;
  * Device: every env of a learner in HBM, stepped, rendered and stacked by one kernel per macro-step
    (mt_<game>_reset / mt_<game>_step) — the device runner of PAACLearner.

Both key an env's draws on (seed, global env id), so they play the same games. A game module (catch.py,
bricks.py, tetris.py) holds its description and re-exports the faces under the game's own names; games()
is the registry that EnvironmentCreator and the tools look a game up in.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib
from .environment import BaseEnvironment


def games():
    """The registry: name -> Game of every device game, in the order the games were added."""
    from . import catch, bricks, tetris
    return OrderedDict((m.GAME.name, m.GAME) for m in (catch, bricks, tetris))


class Game(object):
    """A device game's description.
    defaults: the config's fields in the struct's order -> default value (the keywords of config() and of
      both faces); max_episode_nexts(cfg): an upper bound on the next() calls of one episode;
    from_args(args) -> {keyword: value}: config keywords the command line sets by a rule of its own; every
      other keyword k is read from the flag --<name>_<k>;
    reference: the reference's own game (its rule is not this project's)."""

    def __init__(self, name, num_actions, defaults, max_episode_nexts, from_args=None, reference=False):
        self.name, self.num_actions, self.reference = name, int(num_actions), bool(reference)
        self.defaults = OrderedDict(defaults)
        self.max_episode_nexts = max_episode_nexts
        self.from_args = from_args or (lambda args: {})
        self.config_class = getattr(_lib, 'mt_%s_config' % name)
        self.state_class = getattr(_lib, 'mt_%s_state' % name)
        self.state_bytes = C.sizeof(self.state_class)
        self.state_dtype = np.dtype(self.state_class)  # the record's fields under their C names
        assert self.state_dtype.itemsize == self.state_bytes
        self.symbols = {fn: 'mt_%s_%s' % (name, fn) for fn in _lib.GAME_ENTRY_POINTS}
        title = name.capitalize()
        self.Emulator = type(title + 'Emulator', (Emulator,), {'game': self, '__doc__': Emulator.__doc__})
        self.Device = type(title + 'Device', (Device,), {'game': self, '__doc__': Device.__doc__})

    def config(self, *values, **named):
        """The game's config struct: its fields by position or by keyword, the rest at their defaults."""
        named.update(zip(self.defaults, values))
        if len(values) > len(self.defaults) or set(named) - set(self.defaults):
            raise TypeError('%s config takes %s' % (self.name, ', '.join(self.defaults)))
        return self.config_class(*(int(named.get(k, d)) for k, d in self.defaults.items()))

    def config_from_args(self, args):
        """The config keywords an argparse namespace (train.py's flags) asks for."""
        kw = {k: int(getattr(args, '%s_%s' % (self.name, k), d)) for k, d in self.defaults.items()}
        kw.update(self.from_args(args))
        return kw

    def _call(self, fn, *args):
        _lib.check(getattr(_lib.hip(), self.symbols[fn])(*args), self.symbols[fn])

    def host_reset(self, cfg, seed, global_env, depth, state, out=None):
        """A new game (its draw counter at 0) into `state`; out (84, 84, 4*depth) uint8 or None."""
        self._call('reset_host', C.byref(cfg), C.c_uint64(seed), C.c_uint64(global_env), depth, C.byref(state),
                   None if out is None else out.ctypes.data_as(C.c_void_p))

    def host_step(self, cfg, seed, global_env, depth, tab_rep, a, r, state, prev=None, out=None, frames=None):
        """One macro-step on the host. tab_rep: contiguous int32 array. Returns (reward, over, pushes)."""
        p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        rw, ov, cnt = C.c_float(), C.c_float(), C.c_int32()
        self._call('step_host', C.byref(cfg), C.c_uint64(seed), C.c_uint64(global_env), depth, p(tab_rep), len(tab_rep),
                   int(a), int(r), C.byref(state), p(prev), p(out), p(frames), C.byref(cnt), C.byref(rw), C.byref(ov))
        return rw.value, ov.value != 0.0, cnt.value


class Emulator(BaseEnvironment):
    """The reference's emulator contract: next(action) -> (stacked observation, reward, is_terminal).
    An episode end starts the next game at once (the rule's macro-step), so the observation returned
    with is_terminal is already the new game's initial state, which get_initial_state() then hands
    out again without playing anything (emulator_runner.py:24-41 calls it right after)."""

    game = None  # set by the per-game subclass (Game.Emulator)
    _ONE = np.zeros(1, dtype=np.int32)  # the repetition table of a single next()

    def __init__(self, global_env_id, seed=0, rgb=False, **config):
        self.depth = 3 if rgb else 1
        self.global_env = int(global_env_id)
        self.seed = int(seed)
        self.cfg = self.game.config(**config)
        self.state = self.game.state_class()
        self.obs = np.zeros((84, 84, 4 * self.depth), dtype=np.uint8)
        self._fresh = False  # obs is an initial state nobody asked for yet

    def get_initial_state(self):
        if not self._fresh:  # the first game (or a restart asked for mid-episode): from draw counter 0
            self.game.host_reset(self.cfg, self.seed, self.global_env, self.depth, self.state, self.obs)
        self._fresh = False
        return self.obs.copy()

    def next(self, action):
        out = np.empty_like(self.obs)
        reward, over, _ = self.game.host_step(self.cfg, self.seed, self.global_env, self.depth, self._ONE, action, 0,
                                              self.state, self.obs, out)
        self.obs = out
        self._fresh = over
        return out.copy(), reward, over

    def get_legal_actions(self):
        return np.arange(self.game.num_actions)

    def get_noop(self):
        return 0

    def max_episode_nexts(self):
        return self.game.max_episode_nexts(self.cfg)


class Device(object):
    """Envs [env0, env0 + E) in device memory: owns the state buffer and the repetition table."""

    game = None  # set by the per-game subclass (Game.Device)

    def __init__(self, E, tab_rep, seed=0, env0=0, rgb=False, device='cuda', **config):
        import torch
        self.E, self.env0, self.seed = int(E), int(env0), int(seed)
        self.depth = 3 if rgb else 1
        self.cfg = self.game.config(**config)
        self.tab_rep = torch.tensor(list(tab_rep), dtype=torch.int32, device=device)
        self.R = int(self.tab_rep.numel())
        self.state = torch.zeros(self.E, self.game.state_bytes, dtype=torch.uint8, device=device)
        # (step() is on the learner's host path: the entry points are looked up once)
        self._reset, self._step = (getattr(_lib.hip(), self.game.symbols[fn]) for fn in ('reset', 'step'))

    def reset(self, out):
        """A new game for every env; out [E][84][84][4*depth] receives the stacked initial states."""
        from .network import _ptr, _stream
        assert out.is_contiguous() and out.numel() == self.E * 84 * 84 * 4 * self.depth
        _lib.check(self._reset(C.byref(self.cfg), C.c_uint64(self.seed), self.env0, self.E, self.depth,
                               _ptr(self.state), _ptr(out), _stream()), self.game.symbols['reset'])

    def step(self, a_idx, r_idx, prev, out, reward, over, rm, t, T, frames=None, push_count=None):
        """One macro-step of every env (enqueued on the current stream; no sync): a_idx, r_idx [E] int32,
        prev -> out stacked states, reward / over [E] fp32, rm [2][T][E] fp32 (row t written)."""
        from .network import _ptr, _stream
        assert prev.is_contiguous() and out.is_contiguous() and rm.is_contiguous()
        _lib.check(self._step(C.byref(self.cfg), C.c_uint64(self.seed), self.env0, self.E, self.depth,
                              _ptr(self.tab_rep), self.R, _ptr(a_idx), _ptr(r_idx), _ptr(self.state), _ptr(prev),
                              _ptr(out), _ptr(frames), _ptr(push_count), _ptr(reward), _ptr(over), _ptr(rm), int(t),
                              int(T), _stream()), self.game.symbols['step'])

    def state_array(self):
        """The envs' states as a host array of the game's state records (synchronises)."""
        return np.frombuffer(self.state.cpu().numpy().tobytes(), dtype=self.game.state_dtype)

    def max_episode_nexts(self):
        return self.game.max_episode_nexts(self.cfg)
