"""The device book on the GPU: mt_book_rollout against its host restatement bit for bit (every output and
every persistent word), ring wrap and overflow, capture and replay; then the learner under
--iteration_graph (one replayed graph per training iteration, drained every K) against the asynchronous
eager path: parameters, RMSProp slots, states, indices, episode records, global_step, the LR word, the
final checkpoint of train(), and no host synchronisation between drains."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import test_device_book_cpu as cpu
from manette_amd import _lib
from manette_amd.bookkeeping import DeviceBook

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 3


class Rig(object):
    """A DeviceBook with fixed [T][E] input tensors, beside a HostBook fed the same rollouts."""

    def __init__(self, E, T, R, capacity, env_offset=0, envs_total=None, gs=12345):
        self.E, self.T, self.R = E, T, R
        self.dev = DeviceBook(E, A, cpu.TABS[R], capacity, 0.0224, 80000000.0)
        self.host = cpu.HostBook(E, A, R, capacity, env_offset, envs_total)
        if envs_total is not None:
            self.dev.set_shard(env_offset, envs_total)
        self.dev.set_global_step(gs)
        self.host.words['global_step'] = gs
        self.host.hist[...] = 0  # (the device block starts as zeros)
        self.host.lr[...] = 0
        z = lambda dt: torch.zeros(T, E, dtype=dt, device='cuda')
        self.a, self.r, self.reward, self.over = z(torch.int32), z(torch.int32), z(torch.float32), z(torch.float32)

    def load(self, a, r, reward, over):
        for dst, src in ((self.a, a), (self.r, r), (self.reward, reward), (self.over, over)):
            dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))

    def rollout(self, a, r, reward, over):
        self.load(a, r, reward, over)
        self.dev.rollout(self.a, self.r, self.reward, self.over, self.T)
        self.host.rollout(a, r, reward, over)

    def device_state(self):
        torch.cuda.synchronize()
        d = self.dev
        blk = d.block.cpu().numpy()
        return dict(words=blk[:40].copy().view(cpu.WORDS_DTYPE), lr=blk[40:44].copy().view(np.uint32),
                    hist=blk[d.HIST_OFF:d.ring_off].copy().view(np.int64).reshape(A, self.R),
                    ring=blk[d.ring_off:].copy().view(np.uint8), total=d.total_episode_rewards.cpu().numpy().view(np.uint32),
                    steps=d.emulator_steps.cpu().numpy())

    def host_state(self):
        h = self.host
        return dict(words=h.words.copy(), lr=h.lr.view(np.uint32).copy(), hist=h.hist.copy(),
                    ring=h.ring.view(np.uint8).copy(), total=h.total.view(np.uint32).copy(), steps=h.steps.copy())

    def assert_same(self, where=''):
        got, want = self.device_state(), self.host_state()
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg='%s %s' % (k, where))


@pytest.mark.parametrize('E', [5, 64, 70, 300])  # under a wave, one wave, across waves, two chunks of the block
@pytest.mark.parametrize('R', [1, 11])
@pytest.mark.parametrize('shard', [False, True])
def test_kernel_equals_host_restatement(E, R, shard):
    T = 5
    rig = Rig(E, T, R, 4 * T * E, *((3, E + 11) if shard else (0, None)))
    rs = np.random.RandomState(100 * E + R)
    for k, (density, wild) in enumerate([(0.3, False), (1.1, False), (-1.0, False), (0.3, True)]):
        rig.rollout(*cpu.draw(rs, T, E, A, R, density, wild))
        rig.assert_same('rollout %d' % k)
    assert int(rig.host.words['written'][0]) > T * E


def test_ring_wrap_and_overflow():
    """capacity = T*E and every env ending at every step: with a drain (the ack) between the calls each
    lap overwrites the last; without one the next record sets the flag, appends nothing, overwrites
    nothing, global_step and the LR word still advance, and the next drain raises."""
    E, T, R = 70, 5, 11
    rig = Rig(E, T, R, T * E, gs=0)
    rs = np.random.RandomState(5)
    ones = np.ones((T, E), np.float32)
    for k in range(3):
        a, r, reward, _ = cpu.draw(rs, T, E, A, R, 0.0)
        over = ones.copy()
        if k == 1:
            over[2, 65] = 0  # a lap that ends mid-ring
        rig.rollout(a, r, reward, over)
        rig.assert_same('lap %d before the ack' % k)
        n = len(rig.dev.episodes)
        assert rig.dev.drain() == (k + 1) * T * E
        rig.host.ack()
        assert rig.dev.episodes[n:] == rig.host.records(int(rig.host.words['written'][0]) - int(over.sum()),
                                                        int(rig.host.words['written'][0]))
        rig.assert_same('lap %d' % k)
    rig.rollout(a, r, reward, ones)  # fills the ring; no ack
    one = np.zeros((T, E), np.float32)
    one[4, 69] = 1
    rig.rollout(a, r, reward, one)
    rig.assert_same('overflow')
    w = rig.device_state()['words'][0]
    assert int(w['overflow']) == 1 and int(w['global_step']) == 5 * T * E
    with pytest.raises(_lib.MTError, match='overflow'):
        rig.dev.drain()


def test_capture_and_replay():
    """mt_book_rollout captured once and replayed 3 times == three eager calls: the inputs are read and
    the book advances at replay time."""
    lib = _lib.hip()
    E, T, R = 70, 5, 11
    g_rig, e_rig = Rig(E, T, R, 3 * T * E), Rig(E, T, R, 3 * T * E)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sp = C.c_void_p(side.cuda_stream)
        _lib.check(lib.mt_graph_begin(sp), 'mt_graph_begin')
        g_rig.dev.rollout(g_rig.a, g_rig.r, g_rig.reward, g_rig.over, T)
        graph = C.c_void_p()
        _lib.check(lib.mt_graph_end(sp, C.byref(graph)), 'mt_graph_end')
    try:
        assert int(g_rig.device_state()['words']['global_step'][0]) == 12345  # nothing ran while capturing
        rs = np.random.RandomState(9)
        for k in range(3):
            inputs = cpu.draw(rs, T, E, A, R, 0.3)
            g_rig.load(*inputs)
            g_rig.host.rollout(*inputs)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                _lib.check(lib.mt_graph_launch(graph, C.c_void_p(side.cuda_stream)), 'mt_graph_launch')
            side.synchronize()
            e_rig.rollout(*inputs)
            got, want = g_rig.device_state(), e_rig.device_state()
            for key in want:
                np.testing.assert_array_equal(got[key], want[key], err_msg='%s replay %d' % (key, k))
            g_rig.assert_same('replay %d' % k)
    finally:
        lib.mt_graph_destroy(graph)


# ---- the learner ---------------------------------------------------------------------------------
EC, T = 8, 5


def _learner(tmp, graph, arch='NIPS', max_rep=0, nb=1, rgb=False, drain_every=3, max_global_steps=1 << 40, start=True):
    sys.path.insert(0, ROOT)
    import train as cli
    from manette_amd.exploration_policy import ExplorationPolicy
    from manette_amd.paac import PAACLearner
    a = cli.get_arg_parser().parse_args([])
    a.game, a.arch, a.emulator_counts, a.emulator_workers = 'catch', arch, EC, 0
    a.max_repetition, a.nb_choices, a.rgb = max_rep, nb, rgb
    a.runner, a.sampling, a.seed = 'device', 'device', 0
    a.catch_lives, a.catch_max_balls = 1, 3
    a.iteration_graph, a.drain_every = graph, drain_every
    a.debugging_folder = str(tmp) + '/'
    a.max_global_steps = max_global_steps
    a.checkpoint_interval = 1 << 40
    a.lr_annealing_steps = 100000
    np.random.seed(1234)
    explo = ExplorationPolicy(a)
    nc, ec_ = cli.get_network_and_environment_creator(a, explo)
    L = PAACLearner(nc, ec_, explo, a)
    assert L.max_local_steps == T
    if start:
        L.start()
    return L


def _final(L):
    torch.cuda.synchronize()
    g = lambda x: x.cpu().numpy().copy()
    return dict(params=g(L.network.params), ms=g(L.network.ms), mom=g(L.network.mom), states=g(L.states),
                idx=g(L.idx), gs=L.global_step, episodes=list(L.book.episodes),
                total_rewards=list(L.book.total_rewards), total_steps=list(L.book.total_steps))


@pytest.mark.parametrize('arch,max_rep,nb,rgb', [('NIPS', 0, 1, False), ('NATURE', 10, 11, False),
                                                 ('PWYX', 0, 1, True)])
def test_iteration_graph_equals_eager(tmp_path, arch, max_rep, nb, rgb):
    """7 updates, drain_every 3: one eager iteration, one capture, five replays, two full drains and a
    partial one, against the asynchronous eager path at the same seed."""
    ref = _learner(tmp_path / 'a', False, arch, max_rep, nb, rgb)
    for _ in range(7):
        ref.book.new_update()
        ref.rollout()
        ref.update()
    want = _final(ref)
    want_lr = np.float32(ref.get_lr())
    ref.cleanup()
    L = _learner(tmp_path / 'b', True, arch, max_rep, nb, rgb)
    drains = 0
    for u in range(7):
        L.book.new_update()
        L.rollout()
        lr = L.update()
        if (u + 1) % 3 == 0 or u == 6:
            assert L.drain() == (u + 1) * T * EC
            drains += 1
    assert drains == 3 and L._iter_graph is not None and L._iterations == 7
    got = _final(L)
    lr_word = L.book.lr_value
    L.cleanup()
    for k in ('params', 'ms', 'mom', 'states', 'idx'):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got['gs'] == want['gs'] == 7 * T * EC
    for k in ('episodes', 'total_rewards', 'total_steps'):
        assert got[k] == want[k] and len(want[k]) > 0, k
    assert np.float32(lr) == want_lr and lr_word.view(np.uint32) == want_lr.view(np.uint32)


def _checkpoint(folder):
    d = os.path.join(str(folder), 'checkpoints')
    return {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d))}


def test_train_end_to_end(tmp_path):
    """train() to max_global_steps = 7*T*E, NIPS: both paths stop after the same number of updates and
    leave the same final checkpoint: the step in its name, byte-identical variables."""
    out = {}
    for name, graph in (('eager', False), ('graph', True)):
        L = _learner(tmp_path / name, graph, max_global_steps=7 * T * EC, start=False)
        L.train()
        out[name] = (L.global_step, _checkpoint(tmp_path / name), list(L.book.episodes))
    assert out['graph'][0] == out['eager'][0] == 7 * T * EC
    names = sorted(out['eager'][1])
    assert sorted(out['graph'][1]) == names and '-%d.index' % (7 * T * EC) in names
    for f in names:
        assert out['graph'][1][f] == out['eager'][1][f], f
    assert out['graph'][2] == out['eager'][2] and len(out['eager'][2]) > 0


class _CountingEvent(object):
    def __init__(self, counts):
        self.ev, self.counts = torch.cuda.Event(), counts

    def record(self, *a):
        self.ev.record(*a)

    def synchronize(self):
        self.counts[0] += 1
        self.ev.synchronize()


def test_no_host_synchronisation_between_drains(tmp_path, monkeypatch):
    """Every way the learner waits for the device (its event, a stream's synchronize,
    torch.cuda.synchronize) counted: 0 over K replayed iterations, 1 at the drain."""
    K = 4
    L = _learner(tmp_path, True, drain_every=K)
    try:
        L.rollout()  # eager
        L.rollout()  # captured, launched
        L.drain()
        counts = [0]
        L.event = L.book.event = _CountingEvent(counts)
        real_sync, real_stream_sync = torch.cuda.synchronize, torch.cuda.Stream.synchronize

        def sync(*a, **k):
            counts[0] += 1
            return real_sync(*a, **k)

        def stream_sync(self):
            counts[0] += 1
            return real_stream_sync(self)

        monkeypatch.setattr(torch.cuda, 'synchronize', sync)
        monkeypatch.setattr(torch.cuda.Stream, 'synchronize', stream_sync)
        for _ in range(K):
            L.book.new_update()
            L.rollout()
            L.update()
        assert counts[0] == 0
        assert L.drain() == (2 + K) * T * EC
        assert counts[0] == 1
        monkeypatch.undo()
    finally:
        L.cleanup()
