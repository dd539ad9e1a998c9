"""The device book's rule without a GPU: mt_book_rollout_host (include/manette_hip.h, "Device
bookkeeping") against Bookkeeper.step replayed step by step, exactly; the LR word against get_lr; the
ring's wrap and overflow guard; argument refusals; the --iteration_graph refusals of check_arch_flags."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from manette_amd import _lib
from manette_amd.bookkeeping import EPISODE_DTYPE, WORDS_DTYPE, Bookkeeper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REWARDS = np.array([-3, -1, -0.5, 0, 0.5, 1, 2.5], np.float32)
TABS = {1: [0], 11: [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]}


class HostBook(object):
    """The persistent state of the book in numpy arrays, advanced by mt_book_rollout_host."""

    def __init__(self, E, A, R, capacity, env_offset=0, envs_total=None, initial_lr=0.0224, ann=80000000.0):
        self.E, self.A, self.R, self.capacity = E, A, R, capacity
        self.env_offset, self.envs_total = env_offset, E if envs_total is None else envs_total
        self.initial_lr, self.ann = initial_lr, ann
        self.tab = np.asarray(TABS[R], np.int32)
        self.total = np.zeros(E, np.float32)
        self.steps = np.zeros(E, np.int64)
        self.words = np.zeros(1, WORDS_DTYPE)
        self.hist = np.full((A, R), -7, np.int64)  # (written, not accumulated: stale values must go)
        self.lr = np.full(1, -1, np.float32)
        self.ring = np.zeros(capacity, EPISODE_DTYPE)
        p = lambda x: x.ctypes.data
        self.state = _lib.mt_book_state(p(self.total), p(self.steps), p(self.words), p(self.hist), p(self.lr),
                                        p(self.ring), capacity)

    def args(self, a, r, reward, over, T):
        self._keep = [np.ascontiguousarray(a, np.int32), np.ascontiguousarray(r, np.int32),
                      np.ascontiguousarray(reward, np.float32), np.ascontiguousarray(over, np.float32)]
        return [C.byref(self.state)] + [C.c_void_p(x.ctypes.data) for x in self._keep] + [
            C.c_void_p(self.tab.ctypes.data), self.A, self.R, self.E, T, self.env_offset, self.envs_total,
            self.initial_lr, self.ann]

    def rollout(self, a, r, reward, over):
        _lib.check(_lib.hip().mt_book_rollout_host(*self.args(a, r, reward, over, a.shape[0])), 'mt_book_rollout_host')

    def ack(self):
        self.words['acked'] = self.words['written']

    def records(self, first, last):
        return [(int(x['global_step']), float(x['reward']), int(x['length']))
                for x in (self.ring[k % self.capacity] for k in range(first, last))]


def draw(rs, T, E, A, R, density, wild=False):
    """One rollout's inputs; wild: indices outside their ranges (used clamped)."""
    a = rs.randint(-2 if wild else 0, A + (2 if wild else 0), (T, E)).astype(np.int32)
    r = rs.randint(-2 if wild else 0, R + (2 if wild else 0), (T, E)).astype(np.int32)
    reward = REWARDS[rs.randint(0, len(REWARDS), (T, E))]
    over = (rs.rand(T, E) < density).astype(np.float32)
    return a, r, reward, over


def replay(book, gs, a, r, reward, over):
    """Bookkeeper.step for t = 0 .. T-1 on the clamped indices; returns the new global_step."""
    E = a.shape[1]
    scratch = np.zeros(E, np.float32), np.zeros(E, np.float32)
    book.new_update()
    for t in range(a.shape[0]):
        gs = book.step(gs, np.clip(a[t], 0, book.A - 1), np.clip(r[t], 0, book.R - 1), reward[t], over[t], *scratch)
    return gs


@pytest.mark.parametrize('E', [1, 5, 70])
@pytest.mark.parametrize('T', [1, 5])
@pytest.mark.parametrize('R', [1, 11])
@pytest.mark.parametrize('shard', [False, True])
def test_host_restatement_equals_bookkeeper(E, T, R, shard):
    """Four consecutive rollouts (density 0.3, all ones, all zeros, density 0.3 with wild indices): the
    accumulators carry over; episodes (ints and the fp32 reward's bits), accumulators, global_step,
    histogram and nb_actions are the Bookkeeper's after every rollout."""
    A = 3
    off, total = (3, 16) if shard else (0, None)
    if shard and off + E > 16:
        total = off + E + 2
    hb = HostBook(E, A, R, capacity=4 * T * E, env_offset=off, envs_total=total)
    ref = Bookkeeper(E, A, TABS[R])
    if shard:
        ref.set_shard(off, hb.envs_total)
    rs = np.random.RandomState(1000 * E + 10 * T + R)
    gs = 12345
    hb.words['global_step'] = gs
    for k, (density, wild) in enumerate([(0.3, False), (1.1, False), (-1.0, False), (0.3, True)]):
        a, r, reward, over = draw(rs, T, E, A, R, density, wild)
        first = int(hb.words['written'][0])
        n_before = len(ref.episodes)
        gs = replay(ref, gs, a, r, reward, over)
        hb.rollout(a, r, reward, over)
        w = hb.words[0]
        assert int(w['global_step']) == gs and int(w['overflow']) == 0
        want = ref.episodes[n_before:]
        got = hb.records(first, int(w['written']))
        assert len(got) == len(want) == int(over.sum())
        assert [(g, n) for g, _, n in got] == [(g, n) for g, _, n in want]
        np.testing.assert_array_equal(np.array([x for _, x, _ in got], np.float32).view(np.uint32),
                                      np.array([x for _, x, _ in want], np.float32).view(np.uint32))
        np.testing.assert_array_equal(hb.total.view(np.uint32), ref.total_episode_rewards.view(np.uint32))
        np.testing.assert_array_equal(hb.steps, ref.emulator_steps)
        np.testing.assert_array_equal(hb.hist, ref.total_action_rep, err_msg='rollout %d' % k)
        assert int(w['nb_actions']) == ref.nb_actions


class _LR(object):
    """actor_learner.py:get_lr on a bare object."""
    def __init__(self, gs, initial_lr, ann):
        self.global_step, self.initial_lr, self.lr_annealing_steps = gs, initial_lr, ann
    from manette_amd.actor_learner import ActorLearner
    get_lr = ActorLearner.get_lr


@pytest.mark.parametrize('initial_lr,ann', [(0.0224, 80000000), (0.02, 300000000), (0.007, 1000)])
def test_lr_word_equals_get_lr(initial_lr, ann):
    E, T = 5, 2
    for end in (0 + T * E, ann - 1, ann, ann + 1, ann + T * E, ann // 3 + 7):
        hb = HostBook(E, 3, 1, capacity=T * E, initial_lr=initial_lr, ann=float(ann))
        hb.words['global_step'] = end - T * E
        z = np.zeros((T, E))
        hb.rollout(z, z, z, z)
        assert int(hb.words['global_step'][0]) == end
        want = np.float32(_LR(end, initial_lr, ann).get_lr())
        assert hb.lr.view(np.uint32)[0] == want.view(np.uint32), end
    hb = HostBook(E, 3, 1, capacity=T * E, initial_lr=initial_lr, ann=float(ann))
    hb.words['global_step'] = -T * E  # global_step 0 itself
    hb.rollout(z, z, z, z)
    assert hb.lr[0] == np.float32(initial_lr) == np.float32(_LR(0, initial_lr, ann).get_lr())


def test_ring_wraps_with_an_ack_between_calls():
    """capacity = T*E, every env ends at every step: each rollout fills the ring exactly; with an ack
    between the calls the second lap overwrites the first and nothing overflows."""
    E, T = 5, 3
    hb = HostBook(E, 3, 11, capacity=T * E)
    ref = Bookkeeper(E, 3, TABS[11])
    rs = np.random.RandomState(7)
    gs = 0
    for k in range(3):
        a, r, reward, _ = draw(rs, T, E, 3, 11, 0.0)
        over = np.ones((T, E), np.float32)
        if k == 2:
            over[1, 2] = 0  # a lap that ends mid-ring
        n_before = len(ref.episodes)
        gs = replay(ref, gs, a, r, reward, over)
        hb.rollout(a, r, reward, over)
        w = hb.words[0]
        assert int(w['overflow']) == 0 and int(w['written']) == len(ref.episodes)
        assert hb.records(int(w['acked']), int(w['written'])) == ref.episodes[n_before:]
        hb.ack()


def test_overflow_appends_nothing_and_still_advances():
    E, T = 5, 3
    hb = HostBook(E, 3, 1, capacity=T * E)
    rs = np.random.RandomState(8)
    a, r, reward, _ = draw(rs, T, E, 3, 1, 0.0)
    ones = np.ones((T, E), np.float32)
    hb.rollout(a, r, reward, ones)
    ring, written = hb.ring.copy(), int(hb.words['written'][0])
    assert written == T * E and int(hb.words['overflow'][0]) == 0
    one = np.zeros((T, E), np.float32)
    one[2, 4] = 1  # a single record too many, and no ack
    hb.rollout(a, r, reward, one)
    w = hb.words[0]
    assert int(w['overflow']) == 1 and int(w['written']) == written
    np.testing.assert_array_equal(hb.ring, ring)
    assert int(w['global_step']) == 2 * T * E
    assert hb.lr[0] == np.float32(_LR(2 * T * E, hb.initial_lr, hb.ann).get_lr())
    assert hb.total[4] == 0 and hb.steps[4] == 0  # the env's episode still ended
    hb.ack()  # the flag stays set once raised; records fit again
    hb.rollout(a, r, reward, one)
    assert int(hb.words['overflow'][0]) == 1 and int(hb.words['written'][0]) == written + 1


def test_argument_refusals():
    lib = _lib.hip()
    hb = HostBook(4, 3, 1, capacity=8)
    z = np.zeros((2, 4))
    base = hb.args(z, z, z, z, 2)
    assert lib.mt_book_rollout_host(*base) == 0
    # (position, value): NULLs, sizes < 1, a shard outside the job, lr_annealing_steps <= 0
    for i, v in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (6, 0), (7, 0), (8, 0), (9, 0),
                 (10, -1), (11, 3), (13, 0.0), (13, -5.0)):
        bad = list(base)
        bad[i] = v
        assert lib.mt_book_rollout_host(*bad) == 1, i
        assert lib.mt_book_rollout(*(bad + [None])) == 1, i  # the device entry refuses before any launch
    for field in ('total_episode_rewards', 'emulator_steps', 'words', 'hist', 'lr', 'ring'):
        st = _lib.mt_book_state.from_buffer_copy(hb.state)
        setattr(st, field, None)
        assert lib.mt_book_rollout_host(*([C.byref(st)] + base[1:])) == 1, field
    st = _lib.mt_book_state.from_buffer_copy(hb.state)
    st.capacity = 0
    assert lib.mt_book_rollout_host(*([C.byref(st)] + base[1:])) == 1
    assert b'capacity' in lib.mt_last_error()


def _args(extra):
    sys.path.insert(0, ROOT)
    import train as cli
    return cli.get_arg_parser().parse_args(['-g', 'catch', '--iteration_graph'] + extra)


def test_parser_and_accepted_flags():
    from manette_amd.paac import check_arch_flags
    sys.path.insert(0, ROOT)
    import train as cli
    p = cli.get_arg_parser().parse_args([])
    assert p.iteration_graph is False and p.drain_every is None
    for arch in ('NIPS', 'NATURE', 'PWYX'):
        for rgb in ([], ['--rgb']):
            check_arch_flags(_args(['--runner', 'device', '--sampling', 'device', '--arch', arch] + rgb))
    assert _args(['--drain_every', '3']).drain_every == 3


@pytest.mark.parametrize('extra,match', [
    (['--runner', 'device', '--sampling', 'device', '--arch', 'BAYESIAN'], 'mask'),
    (['--runner', 'device', '--sampling', 'device', '--arch', 'LSTM'], 'LSTM'),
    (['--runner', 'device', '--sampling', 'host'], 'sampling'),
    (['--runner', 'python', '--sampling', 'device'], 'runner'),
    (['--runner', 'python', '--sampling', 'host'], 'runner'),
    (['--runner', 'device', '--sampling', 'device', '--drain_every', '0'], 'drain_every'),
])
def test_iteration_graph_refusals(extra, match):
    from manette_amd.paac import check_arch_flags
    with pytest.raises(ValueError, match=match):
        check_arch_flags(_args(extra))


def test_iteration_graph_refuses_more_than_one_process(monkeypatch):
    from manette_amd.paac import check_arch_flags
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='world 1'):
        check_arch_flags(_args(['--runner', 'device', '--sampling', 'device']))
