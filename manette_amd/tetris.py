"""Tetris: the reference's own game (tetris.py / tetris_emulator.py, `-g tetris`: a 10 x 22 board of coloured
cells, seven pieces with four rotations, row removal, levels, five actions), its rule restated in
include/manette_hip.h ("Tetris") and pinned act by act to recordings of the reference's code. Two faces of
the same rule, with the signatures of manette_amd/bricks.py, so the learner has no per-game branch:

  * TetrisEmulator: the reference contract (BaseEnvironment) on the host restatement
    (mt_tetris_reset_host / mt_tetris_step_host, no GPU needed) — the Python runner, test.py, CPU paths;
  * TetrisDevice: every env of a learner in HBM, stepped, rendered and stacked by one kernel per
    macro-step (mt_tetris_reset / mt_tetris_step) — the device runner of PAACLearner.

Both key an env's piece draws on (seed, global env id), so they play the same games.
"""
import ctypes as C

import numpy as np

from . import _lib
from .environment import BaseEnvironment

NUM_ACTIONS = 5
DEFAULT_MAX_NEXTS = 2000
DEFAULT_SPEED = 5
DEFAULT_MAX_START_WAIT = 0
RANDOM_START_WAIT = 30  # tetris_emulator.py's MAX_START_WAIT, under --random_start
STATE_BYTES = C.sizeof(_lib.mt_tetris_state)
STATE_DTYPE = np.dtype([('board', np.uint32, (22,))] +
                       [(n, np.int32) for n in ('piece', 'rot', 'x', 'y', 'next_piece', 'level', 'lines', 'speed',
                                                'speed_counter', 'nexts')] +
                       [('piece_counter', np.uint64)])
assert STATE_DTYPE.itemsize == STATE_BYTES == 136


def config(max_nexts=DEFAULT_MAX_NEXTS, speed=DEFAULT_SPEED, max_start_wait=DEFAULT_MAX_START_WAIT):
    return _lib.mt_tetris_config(int(max_nexts), int(speed), int(max_start_wait))


def max_episode_nexts(cfg):
    """An upper bound on the next() calls of one episode (so on its macro-steps, each of which plays at
    least one): the rule ends an episode when nexts >= max_nexts."""
    return int(cfg.max_nexts)


def host_reset(cfg, seed, global_env, depth, state, out=None):
    """A new game into `state` (piece_counter = 0 first); out (84, 84, 4*depth) uint8 or None."""
    _lib.check(_lib.hip().mt_tetris_reset_host(C.byref(cfg), C.c_uint64(seed), C.c_uint64(global_env), depth,
                                               C.byref(state), None if out is None else out.ctypes.data_as(C.c_void_p)),
               'mt_tetris_reset_host')


def host_step(cfg, seed, global_env, depth, tab_rep, a, r, state, prev=None, out=None, frames=None):
    """One macro-step on the host. tab_rep: contiguous int32 array. Returns (reward, over, pushes)."""
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    rw, ov, cnt = C.c_float(), C.c_float(), C.c_int32()
    _lib.check(_lib.hip().mt_tetris_step_host(C.byref(cfg), C.c_uint64(seed), C.c_uint64(global_env), depth,
                                              p(tab_rep), len(tab_rep), int(a), int(r), C.byref(state), p(prev), p(out),
                                              p(frames), C.byref(cnt), C.byref(rw), C.byref(ov)), 'mt_tetris_step_host')
    return rw.value, ov.value != 0.0, cnt.value


class TetrisEmulator(BaseEnvironment):
    """The reference's emulator contract: next(action) -> (stacked observation, reward, is_terminal).
    An episode end starts the next game at once (the rule's macro-step), so the observation returned
    with is_terminal is already the new game's initial state, which get_initial_state() then hands
    out again without playing anything."""

    _ONE = np.zeros(1, dtype=np.int32)  # the repetition table of a single next()

    def __init__(self, global_env_id, seed=0, rgb=False, max_nexts=DEFAULT_MAX_NEXTS, speed=DEFAULT_SPEED,
                 max_start_wait=DEFAULT_MAX_START_WAIT):
        self.depth = 3 if rgb else 1
        self.global_env = int(global_env_id)
        self.seed = int(seed)
        self.cfg = config(max_nexts, speed, max_start_wait)
        self.state = _lib.mt_tetris_state()
        self.obs = np.zeros((84, 84, 4 * self.depth), dtype=np.uint8)
        self._fresh = False  # obs is an initial state nobody asked for yet

    def get_initial_state(self):
        if not self._fresh:  # the first game (or a restart asked for mid-episode): from piece_counter 0
            host_reset(self.cfg, self.seed, self.global_env, self.depth, self.state, self.obs)
        self._fresh = False
        return self.obs.copy()

    def next(self, action):
        out = np.empty_like(self.obs)
        reward, over, _ = host_step(self.cfg, self.seed, self.global_env, self.depth, self._ONE, action, 0,
                                    self.state, self.obs, out)
        self.obs = out
        self._fresh = over
        return out.copy(), reward, over

    def get_legal_actions(self):
        return np.arange(NUM_ACTIONS)

    def get_noop(self):
        return 0


class TetrisDevice(object):
    """Envs [env0, env0 + E) in device memory: owns the state buffer and the repetition table."""

    def __init__(self, E, tab_rep, seed=0, env0=0, rgb=False, max_nexts=DEFAULT_MAX_NEXTS, speed=DEFAULT_SPEED,
                 max_start_wait=DEFAULT_MAX_START_WAIT, device='cuda'):
        import torch
        self.E, self.env0, self.seed = int(E), int(env0), int(seed)
        self.depth = 3 if rgb else 1
        self.cfg = config(max_nexts, speed, max_start_wait)
        self.tab_rep = torch.tensor(list(tab_rep), dtype=torch.int32, device=device)
        self.R = int(self.tab_rep.numel())
        self.state = torch.zeros(self.E, STATE_BYTES, dtype=torch.uint8, device=device)

    def reset(self, out):
        """A new game for every env; out [E][84][84][4*depth] receives the stacked initial states."""
        from .network import _ptr, _stream
        assert out.is_contiguous() and out.numel() == self.E * 84 * 84 * 4 * self.depth
        _lib.check(_lib.hip().mt_tetris_reset(C.byref(self.cfg), C.c_uint64(self.seed), self.env0, self.E, self.depth,
                                              _ptr(self.state), _ptr(out), _stream()), 'mt_tetris_reset')

    def step(self, a_idx, r_idx, prev, out, reward, over, rm, t, T, frames=None, push_count=None):
        """One macro-step of every env (enqueued on the current stream; no sync): a_idx, r_idx [E] int32,
        prev -> out stacked states, reward / over [E] fp32, rm [2][T][E] fp32 (row t written)."""
        from .network import _ptr, _stream
        assert prev.is_contiguous() and out.is_contiguous() and rm.is_contiguous()
        _lib.check(_lib.hip().mt_tetris_step(C.byref(self.cfg), C.c_uint64(self.seed), self.env0, self.E, self.depth,
                                             _ptr(self.tab_rep), self.R, _ptr(a_idx), _ptr(r_idx), _ptr(self.state),
                                             _ptr(prev), _ptr(out), _ptr(frames), _ptr(push_count), _ptr(reward),
                                             _ptr(over), _ptr(rm), int(t), int(T), _stream()), 'mt_tetris_step')

    def state_array(self):
        """The envs' states as a host array of mt_tetris_state records (synchronises)."""
        return np.frombuffer(self.state.cpu().numpy().tobytes(), dtype=STATE_DTYPE)
