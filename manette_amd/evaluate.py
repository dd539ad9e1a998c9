"""Device-resident evaluation of a policy on a device game (include/manette_hip.h, "Device evaluation").

DeviceEvaluator plays K episodes on each of N envs of a device game with a fixed chooser and a draw
stream of its own, every run on the same games (a run resets the envs, so their draw streams
start from counter 0 again). A macro-step is forward (infer) -> draw -> env kernel -> mt_eval_step, all
enqueued; the host looks at the device's word block once per `check_every` steps. The per-episode
results stay in device tables until the run ends; mt_eval_summarize reduces them in a fixed order.

It shares nothing writable with a learner: its own env, state buffers, draw counters, workspace key
('eval') and eval state, and it only reads the parameter buffer. BAYESIAN keeps dropout on (as test.py
does) from the 'eval' workspace's own dropout state; LSTM runs on an [N][5][frame] memory advanced by
mt_memory_push after each env step (a window is zeroed at an episode end, as in training).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import network as devnet
from .network import _ptr, _stream

EVAL_ENV0 = 1 << 20        # global env id of a learner's evaluation env 0: disjoint from every training env
EVAL_SEED_SALT = 0x4556414c44524157  # a learner's evaluation draw seed = sample_seed ^ this

WORDS_DTYPE = np.dtype([('remaining', np.int64), ('steps', np.int64)])
SUMMARY_DTYPE = np.dtype([('episodes', np.int64), ('unfinished', np.int64), ('length_sum', np.int64),
                          ('sum', np.float64), ('sumsq', np.float64), ('min', np.float32), ('max', np.float32),
                          ('pad', np.int32, (2,))])
assert WORDS_DTYPE.itemsize == C.sizeof(_lib.mt_eval_words) == 16
assert SUMMARY_DTYPE.itemsize == C.sizeof(_lib.mt_eval_summary) == 56


def state_layout(N, K):
    """{name: (byte offset, bytes)} and the total of the one allocation that holds an eval state: the
    word block first (what a check copies), then the summary, the accumulators and the two tables, every
    offset a multiple of 16."""
    up = lambda x: -(-x // 16) * 16
    off, out = 0, {}
    for name, n in (('words', 16), ('summary', 56), ('ret_acc', 4 * N), ('len_acc', 8 * N), ('done', 4 * N),
                    ('returns', 4 * N * K), ('lengths', 8 * N * K)):
        out[name] = (off, n)
        off = up(off + n)
    return out, off


def make_state(base, N, K):
    """The mt_eval_state of a block laid out by state_layout at address `base` (device or host)."""
    lay, _ = state_layout(N, K)
    at = lambda k: base + lay[k][0]
    return _lib.mt_eval_state(at('ret_acc'), at('len_acc'), at('done'), at('returns'), at('lengths'), at('words'),
                              int(N), int(K))


class EvalResult(object):
    """One evaluation: the statistics of the finished episodes and the tables they came from."""

    def __init__(self, summary, returns, lengths, done, macro_steps, trace=None):
        self.episodes = int(summary['episodes'])
        self.unfinished = int(summary['unfinished'])
        self.sum, self.sumsq = float(summary['sum']), float(summary['sumsq'])
        n = self.episodes
        self.mean = self.sum / n if n else 0.0
        # the population deviation, as np.std (the difference of two close numbers may round below zero)
        self.std = float(np.sqrt(max(self.sumsq / n - self.mean * self.mean, 0.0))) if n else 0.0
        self.min, self.max = float(summary['min']), float(summary['max'])
        self.mean_length = float(summary['length_sum']) / n if n else 0.0
        self.returns, self.lengths, self.done = returns, lengths, done  # [N][K], [N][K], [N]
        self.macro_steps = int(macro_steps)
        self.trace = trace  # record=True: [steps][2][N] int32 (action, repetition indices)

    def finished(self):
        """The finished episodes' returns, env-major (what the summary covers)."""
        K = self.returns.shape[1]
        return self.returns[np.arange(K)[None, :] < self.done[:, None]]

    def __repr__(self):
        return ('EvalResult(episodes=%d, unfinished=%d, mean=%.4f, std=%.4f, min=%.2f, max=%.2f, mean_length=%.2f, '
                'macro_steps=%d)' % (self.episodes, self.unfinished, self.mean, self.std, self.min, self.max,
                                     self.mean_length, self.macro_steps))


class DeviceEvaluator(object):
    def __init__(self, network, env_creator, tab_rep, n_envs, episodes=1, policy=None, draw_seed=0, env0=None,
                 graph=True, check_every=32, max_macro_steps=None, record=False):
        N, K = int(n_envs), int(episodes)
        if N < 1 or K < 1:
            raise ValueError('DeviceEvaluator: n_envs and episodes must be >= 1')
        self.network, self.N, self.K = network, N, K
        dev = network.device
        self.env = env_creator.create_device_env(N, tab_rep, device=dev)
        if env0 is not None:
            self.env.env0 = int(env0)
        self.policy = policy
        self.draw_seed = int(draw_seed) & 0xffffffffffffffff
        self.graph = bool(graph)
        self.check_every = max(2, int(check_every) + (int(check_every) & 1))  # even: the ping-pong parity closes
        self.max_macro_steps = K * self.env.max_episode_nexts() + 1 if max_macro_steps is None else int(max_macro_steps)
        self.record = bool(record)
        self.lstm = network.arch == 'LSTM'
        self.bayes = network.arch == 'BAYESIAN'
        Cn = 4 * self.env.depth
        A, R = network.num_actions, self.env.R
        self.states = torch.zeros(2, N, 84, 84, Cn, dtype=torch.uint8, device=dev)
        if self.lstm:
            self.memory = torch.zeros(N, 5, 84, 84, Cn, dtype=torch.uint8, device=dev)
            self._whole = torch.zeros_like(self.memory)  # mt_memory_push's copy of the window (unused here)
        self.out = (torch.zeros(N, dtype=torch.float32, device=dev), torch.zeros(N, A, dtype=torch.float32, device=dev),
                    torch.zeros(N, R, dtype=torch.float32, device=dev))
        self.counters = torch.zeros(N, dtype=torch.int64, device=dev)
        self.idx = torch.zeros(self.check_every, 2, N, dtype=torch.int32, device=dev)  # one block's draws
        self.ro = torch.zeros(2, N, dtype=torch.float32, device=dev)                   # [0] rewards, [1] over flags
        self.rm = torch.zeros(2, 1, N, dtype=torch.float32, device=dev)                # the env kernel's T = 1 scratch
        self.layout, nbytes = state_layout(N, K)
        self.block = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self._pin = torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True)
        self.state = make_state(self.block.data_ptr(), N, K)
        self._summary_addr = self.block.data_ptr() + self.layout['summary'][0]
        self.event = torch.cuda.Event()
        self._graph = None
        self._graph_stream = None
        network.workspace(N, 'eval')

    # ------------------------------------------------------------------------------------------
    def _macro_step(self, j):
        """Macro-step j of a block: states[j % 2] -> states[(j + 1) % 2], the draw into idx[j]."""
        net, env, N = self.network, self.env, self.N
        prev, nxt = self.states[j & 1], self.states[(j + 1) & 1]
        _, pi, rep = net.forward(self.memory if self.lstm else prev, N, out=self.out, ws_key='eval', infer=True)
        a, r = self.idx[j, 0], self.idx[j, 1]
        devnet.sample(pi, rep, self.draw_seed, self.counters, a, r, row0=env.env0, policy=self.policy)
        env.step(a, r, prev, nxt, self.ro[0], self.ro[1], self.rm, 0, 1)
        _lib.check(_lib.hip().mt_eval_step(C.byref(self.state), _ptr(r), _ptr(self.ro[0]), _ptr(self.ro[1]),
                                           _ptr(env.tab_rep), env.R, _stream()), 'mt_eval_step')
        if self.lstm:  # masks = 1 - over, as the env kernel left them in its rm scratch
            devnet.memory_push(self.memory, self._whole, nxt, self.rm[1, 0])

    def _block(self, n):
        for j in range(n):
            self._macro_step(j)

    def _capture(self):
        lib = _lib.hip()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            sp = _stream()
            _lib.check(lib.mt_graph_begin(sp), 'mt_graph_begin')
            try:
                self._block(self.check_every)
            finally:
                g = C.c_void_p()
                rc = lib.mt_graph_end(sp, C.byref(g))
            _lib.check(rc, 'mt_graph_end')
        self._graph, self._graph_stream = g, side
        self._graph_ws = self.network.workspace(self.N, 'eval').data_ptr()

    def _words(self):
        """The word block as of now: one 16-byte D2H copy and one synchronisation."""
        self._pin[:16].copy_(self.block[:16], non_blocking=True)
        self.event.record()
        self.event.synchronize()
        w = self._pin[:16].numpy().view(WORDS_DTYPE)[0]
        return int(w['remaining']), int(w['steps'])

    def run(self):
        """Play the evaluation; returns an EvalResult. Deterministic: the same games, the same draws."""
        lib, net = _lib.hip(), self.network
        # (the 'eval' workspace belongs to the network: a larger evaluator on the same network replaces it,
        # and a graph captured on the old one must not be replayed)
        if self._graph is not None and net.workspace(self.N, 'eval').data_ptr() != self._graph_ws:
            self.close()
        self.env.reset(self.states[0])
        self.counters.zero_()
        if self.bayes:  # dropout stays on, from this workspace's own stream (restarted: the same masks every run)
            net.set_dropout_state('eval', self.draw_seed ^ 0x4556414c44524f50, self.env.env0, batch=self.N)
        if self.lstm:   # memory = zeros except memory[:, -1] = the initial state
            self.memory.zero_()
            self.memory[:, 4].copy_(self.states[0])
        _lib.check(lib.mt_eval_reset(C.byref(self.state), _stream()), 'mt_eval_reset')
        trace, steps, blocks, remaining = [], 0, 0, self.N * self.K
        while remaining > 0 and steps < self.max_macro_steps:
            n = min(self.check_every, self.max_macro_steps - steps)
            whole = n == self.check_every
            if whole and self.graph and self._graph is None and blocks >= 1:
                self._capture()
            if whole and self._graph is not None:
                _lib.check(lib.mt_graph_launch(self._graph, _stream()), 'mt_graph_launch')
            else:
                self._block(n)
            blocks += 1
            steps += n
            if self.record:
                trace.append(self.idx[:n].cpu().numpy().copy())
            remaining, counted = self._words()
            if counted != steps:
                raise _lib.MTError('device evaluation: %d steps counted on the device, %d enqueued' % (counted, steps))
        _lib.check(lib.mt_eval_summarize(C.byref(self.state), C.c_void_p(self._summary_addr), _stream()),
                   'mt_eval_summarize')
        self._pin.copy_(self.block, non_blocking=True)
        self.event.record()
        self.event.synchronize()
        host = self._pin.numpy()
        cut = lambda k, dt: host[self.layout[k][0]:self.layout[k][0] + self.layout[k][1]].view(dt).copy()
        return EvalResult(cut('summary', SUMMARY_DTYPE)[0], cut('returns', np.float32).reshape(self.N, self.K),
                          cut('lengths', np.int64).reshape(self.N, self.K), cut('done', np.int32), steps,
                          np.concatenate(trace) if self.record and trace else None)

    def close(self):
        if self._graph is not None:
            torch.cuda.synchronize()
            _lib.hip().mt_graph_destroy(self._graph)
            self._graph = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def policy_from_args(args, greedy=False, rows_per_call=1):
    """The chooser of an evaluation: argmax with `greedy`, else what the run's args imply, as
    PAACLearner.__init__ builds it (None = multinomial, or the e-greedy settings)."""
    if greedy:
        return _lib.mt_policy(_lib.MT_POLICY['argmax'], 0, 0.0, 0.0, 1)
    if getattr(args, 'egreedy', False):
        return _lib.mt_policy(_lib.MT_POLICY['egreedy'], int(bool(getattr(args, 'annealed', False))),
                              float(getattr(args, 'epsilon', 0.05)), float(getattr(args, 'annealed_steps', 80000000)),
                              int(rows_per_call))
    return None
