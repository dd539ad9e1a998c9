"""Catch on the GPU: the env kernel (mt_catch_step: step, render and stack in one launch) against the
host restatement bit for bit, its fused stack against the existing stacking kernel, launch splits,
graph capture, and the learner's device runner against its lockstep form and the reference-contract
Python runner."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import catch_ref
from manette_amd import _lib, catch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234567
TABS = {1: [0], 11: catch_ref.tab_repetitions(10, 11)}


class Rig(object):
    """A CatchDevice with its buffers; step(a, r) plays one macro-step prev -> out and swaps them."""

    def __init__(self, E, R, depth=1, lives=3, max_balls=20, env0=0, T=3, frames=True):
        self.E, self.R, self.depth, self.env0, self.T, self.t = E, R, depth, env0, T, 0
        self.lives, self.max_balls = lives, max_balls
        self.dev = catch.CatchDevice(E, TABS[R], seed=SEED, env0=env0, rgb=depth == 3, lives=lives,
                                     max_balls=max_balls)
        z = lambda *s, **k: torch.zeros(*s, device='cuda', **k)
        self.bufs = [z(E, 84, 84, 4 * depth, dtype=torch.uint8), z(E, 84, 84, 4 * depth, dtype=torch.uint8)]
        self.a, self.r = z(E, dtype=torch.int32), z(E, dtype=torch.int32)
        self.reward, self.over, self.rm = z(E), z(E), z(2, T, E)
        self.frames = z(4 * E, 84, 84, depth, dtype=torch.uint8) if frames else None
        self.count = z(E, dtype=torch.int32) if frames else None
        self.dev.reset(self.bufs[0])

    @property
    def obs(self):
        return self.bufs[0]

    def step(self, a, r):
        self.a.copy_(torch.as_tensor(np.asarray(a, np.int32)))
        self.r.copy_(torch.as_tensor(np.asarray(r, np.int32)))
        self.dev.step(self.a, self.r, self.bufs[0], self.bufs[1], self.reward, self.over, self.rm, self.t, self.T,
                      self.frames, self.count)
        t = self.t
        self.bufs.reverse()
        self.t = (t + 1) % self.T
        return t

    def outputs(self, t):
        g = lambda x: x.cpu().numpy().copy()
        return dict(obs=g(self.obs), reward=g(self.reward), over=g(self.over), clipped=g(self.rm[0, t]),
                    mask=g(self.rm[1, t]), state=self.dev.state_array().copy(),
                    frames=None if self.frames is None else g(self.frames),
                    count=None if self.count is None else g(self.count))


class HostRig(object):
    """The same envs on mt_catch_*_host."""

    def __init__(self, E, R, depth=1, lives=3, max_balls=20, env0=0):
        self.E, self.depth, self.env0 = E, depth, env0
        self.tab = np.asarray(TABS[R], np.int32)
        self.cfg = catch.config(lives, max_balls)
        self.st = [_lib.mt_catch_state() for _ in range(E)]
        self.obs = np.zeros((E, 84, 84, 4 * depth), np.uint8)
        for e in range(E):
            catch.host_reset(self.cfg, SEED, env0 + e, depth, self.st[e], self.obs[e])

    def step(self, a, r):
        E = self.E
        out = np.empty_like(self.obs)
        res = dict(reward=np.zeros(E, np.float32), over=np.zeros(E, np.float32), count=np.zeros(E, np.int32),
                   frames=np.zeros((4 * E, 84, 84, self.depth), np.uint8))
        for e in range(E):
            rw, ov, cnt = catch.host_step(self.cfg, SEED, self.env0 + e, self.depth, self.tab, a[e], r[e], self.st[e],
                                          self.obs[e], out[e], res['frames'][4 * e:4 * e + 4])
            res['reward'][e], res['over'][e], res['count'][e] = rw, ov, cnt
        self.obs = out
        res.update(obs=out, clipped=np.clip(res['reward'], -1, 1), mask=1 - res['over'],
                   state=np.frombuffer(b''.join(bytes(s) for s in self.st), dtype=catch.STATE_DTYPE))
        return res


def _actions(step, E, R, wild=False):
    ar = [catch_ref.hashed_actions(step, e, R) for e in range(E)]
    a, r = [x for x, _ in ar], [y for _, y in ar]
    if wild:  # out-of-range indices: clamped in the kernel as on the host
        a[0], r[0], a[1], r[1] = -3, -7, 11, 10 ** 6
    return a, r


def _assert_same(got, want, frames=True, where=''):
    for k in ('reward', 'over', 'clipped', 'mask', 'state', 'obs'):
        np.testing.assert_array_equal(got[k], want[k], err_msg='%s %s' % (k, where))
    if frames:
        np.testing.assert_array_equal(got['count'], want['count'], err_msg='count ' + where)
        for e, c in enumerate(want['count']):  # (slots past the count are not written)
            np.testing.assert_array_equal(got['frames'][4 * e:4 * e + c], want['frames'][4 * e:4 * e + c],
                                          err_msg='frames env %d %s' % (e, where))


@pytest.mark.parametrize('env0', [0, 37])
@pytest.mark.parametrize('lives,max_balls', [(1, 2), (3, 20)])
@pytest.mark.parametrize('R', [1, 11])
@pytest.mark.parametrize('depth', [1, 3])
def test_kernel_matches_host(depth, R, lives, max_balls, env0):
    """Every output of mt_catch_step, 60 macro-steps of E = 5 envs, bit for bit."""
    d = Rig(5, R, depth, lives, max_balls, env0)
    h = HostRig(5, R, depth, lives, max_balls, env0)
    np.testing.assert_array_equal(d.obs.cpu().numpy(), h.obs)
    ended = 0
    for step in range(60):
        a, r = _actions(step, 5, R, wild=step % 7 == 3)
        t = d.step(a, r)
        want = h.step(a, r)
        _assert_same(d.outputs(t), want, where='step %d' % step)
        ended += int(want['over'].sum())
    if (lives, max_balls) == (1, 2) or R == 11:
        assert ended > 0


def _resized_stack(frames, count, prev, E, depth):
    from manette_amd import network as devnet
    out = torch.zeros_like(prev)
    off = torch.arange(0, 4 * E, 4, dtype=torch.int32, device='cuda')
    devnet.preprocess(frames, off, count, E, depth, None, None, prev, out, resized=True)
    return out.cpu().numpy()


@pytest.mark.parametrize('E,depth,steps', [(5, 1, 25), (5, 3, 25), (64, 1, 2)])
def test_fused_stack_equals_preprocess_resized(E, depth, steps):
    """The kernel's render-and-stack pass == mt_preprocess_resized on its frames_out / push_count_out and
    the same prev (FiGAR table: pushes from 1 to more than 4, and resets)."""
    d = Rig(E, 11, depth, 1, 3)
    for step in range(steps):
        a, r = _actions(step, E, 11)
        prev = d.obs
        d.step(a, r)
        want = _resized_stack(d.frames, d.count, prev, E, depth)
        np.testing.assert_array_equal(d.obs.cpu().numpy(), want, err_msg='step %d' % step)


def test_launch_split():
    """E = 8 in one launch == two launches of 4 with env0 = 0 and 4."""
    whole = Rig(8, 11, 1, 1, 3, frames=False)
    parts = [Rig(4, 11, 1, 1, 3, env0=0, frames=False), Rig(4, 11, 1, 1, 3, env0=4, frames=False)]
    for step in range(30):
        a, r = _actions(step, 8, 11)
        t = whole.step(a, r)
        got = whole.outputs(t)
        for i, p in enumerate(parts):
            tp = p.step(a[4 * i:4 * i + 4], r[4 * i:4 * i + 4])
            want = p.outputs(tp)
            for k in ('reward', 'over', 'clipped', 'mask', 'state', 'obs'):
                np.testing.assert_array_equal(got[k][4 * i:4 * i + 4], want[k], err_msg='%s step %d' % (k, step))


def test_capture_and_replay():
    """One captured mt_catch_step replayed 3 times == 3 eager calls: the state advances in device memory
    and the indices are read at replay time, nothing is baked into the graph."""
    lib = _lib.hip()
    g_rig, e_rig = Rig(5, 11, 1, 1, 2), Rig(5, 11, 1, 1, 2)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sp = C.c_void_p(side.cuda_stream)
        _lib.check(lib.mt_graph_begin(sp), 'mt_graph_begin')
        g_rig.dev.step(g_rig.a, g_rig.r, g_rig.bufs[0], g_rig.bufs[1], g_rig.reward, g_rig.over, g_rig.rm, 0, g_rig.T,
                       g_rig.frames, g_rig.count)
        graph = C.c_void_p()
        _lib.check(lib.mt_graph_end(sp, C.byref(graph)), 'mt_graph_end')
    try:
        for k in range(3):
            a, r = _actions(k, 5, 11)
            a[2], r[2] = k % 3, 10  # env 2: 11 nexts per replay, so its game ends within the three
            g_rig.a.copy_(torch.as_tensor(np.asarray(a, np.int32)))
            g_rig.r.copy_(torch.as_tensor(np.asarray(r, np.int32)))
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                _lib.check(lib.mt_graph_launch(graph, C.c_void_p(side.cuda_stream)), 'mt_graph_launch')
            side.synchronize()
            got = dict(obs=g_rig.bufs[1].cpu().numpy(), state=g_rig.dev.state_array().copy(),
                       reward=g_rig.reward.cpu().numpy(), over=g_rig.over.cpu().numpy())
            e_rig.a.copy_(torch.as_tensor(np.asarray(a, np.int32)))
            e_rig.r.copy_(torch.as_tensor(np.asarray(r, np.int32)))
            e_rig.dev.step(e_rig.a, e_rig.r, e_rig.bufs[0], e_rig.bufs[1], e_rig.reward, e_rig.over, e_rig.rm, 0,
                           e_rig.T, e_rig.frames, e_rig.count)
            torch.cuda.synchronize()
            want = dict(obs=e_rig.bufs[1].cpu().numpy(), state=e_rig.dev.state_array().copy(),
                        reward=e_rig.reward.cpu().numpy(), over=e_rig.over.cpu().numpy())
            for key in want:
                np.testing.assert_array_equal(got[key], want[key], err_msg='%s replay %d' % (key, k))
            if k:
                assert (got['state'] != last).any()  # the state advanced between replays
            last = got['state']
    finally:
        lib.mt_graph_destroy(graph)


def test_device_argument_checks():
    d = Rig(4, 1)
    lib = _lib.hip()
    p = lambda t: C.c_void_p(t.data_ptr())
    base = [C.byref(d.dev.cfg), C.c_uint64(1), 0, 4, 1, p(d.dev.tab_rep), 1, p(d.a), p(d.r), p(d.dev.state),
            p(d.bufs[0]), p(d.bufs[1]), None, None, p(d.reward), p(d.over), p(d.rm), 0, 3, None]
    assert lib.mt_catch_step(*base) == 0
    for i, v in ((3, 0), (4, 2), (6, 0), (17, 3), (17, -1), (11, p(d.bufs[0])), (9, None), (16, None),
                 (12, p(d.frames)), (0, C.byref(catch.config(0, 5)))):
        bad = list(base)
        bad[i] = v
        assert lib.mt_catch_step(*bad) == 1, i
    torch.cuda.synchronize()


# ---- the learner ---------------------------------------------------------------------------------
def _learner(tmp, runner, sampling, arch='NIPS', ec=8, max_rep=0, nb=1, seed=0, lives=1, max_balls=3, rgb=False,
             lr=None, lockstep=False):
    sys.path.insert(0, ROOT)
    import train as cli
    from manette_amd.exploration_policy import ExplorationPolicy
    from manette_amd.paac import PAACLearner
    a = cli.get_arg_parser().parse_args([])
    a.game, a.arch, a.emulator_counts, a.emulator_workers = 'catch', arch, ec, 0
    a.max_repetition, a.nb_choices, a.rgb = max_rep, nb, rgb
    a.runner, a.sampling, a.seed = runner, sampling, seed
    a.catch_lives, a.catch_max_balls = lives, max_balls
    a.debugging_folder = str(tmp) + '/'
    a.max_global_steps = 1 << 40
    a.checkpoint_interval = 1 << 40
    a.lr_annealing_steps = 100000
    if lr is not None:
        a.initial_lr, a.lr_annealing_steps = lr, 300000000
    np.random.seed(1234)
    explo = ExplorationPolicy(a)
    nc, ec_ = cli.get_network_and_environment_creator(a, explo)
    L = PAACLearner(nc, ec_, explo, a)
    L.lockstep = lockstep
    L.start()
    return L


def _run(L, updates):
    """Per update: what the rollout left (all state slots, indices, device and host rewards / masks)."""
    trail = []
    for _ in range(updates):
        L.book.new_update()
        L.rollout()
        torch.cuda.synchronize()
        g = lambda x: x.cpu().numpy().copy()
        rec = dict(states=g(L.states), idx=g(L.idx), rm_host=L.rm_h.numpy().copy())
        if L.runner_kind == 'device':
            rec.update(rm_dev=g(L.rm_d))
        trail.append(rec)
        L.update()
    torch.cuda.synchronize()
    return trail


def _final(L):
    g = lambda x: x.cpu().numpy().copy()
    return dict(params=g(L.network.params), ms=g(L.network.ms), mom=g(L.network.mom), gs=L.global_step,
                episodes=list(L.book.episodes))


def _host_replay(L, trail, lives, max_balls):
    """global_step and episode records of the same indices played on CatchEmulators by the
    reference-contract runner loop and the Python bookkeeper."""
    from manette_amd.bookkeeping import Bookkeeper
    from manette_amd.emulator_runner import run_emulators
    E, T = L.emulator_counts, L.max_local_steps
    emus = [catch.CatchEmulator(e, seed=L.seed, rgb=L.depth == 3, lives=lives, max_balls=max_balls) for e in range(E)]
    states = np.asarray([e.get_initial_state() for e in emus])
    var = [states, np.zeros(E, np.float32), np.zeros(E, np.float32), np.zeros(E, np.int32), np.zeros(E, np.int32)]
    book = Bookkeeper(E, 3, L.tab_rep)
    gs, rw, mk = 0, np.zeros(E, np.float32), np.zeros(E, np.float32)
    for rec in trail:
        np.testing.assert_array_equal(rec['states'][0], var[0])
        for t in range(T):
            var[3][...], var[4][...] = rec['idx'][0, t], rec['idx'][1, t]
            run_emulators(L.tab_rep, emus, var)
            gs = book.step(gs, var[3], var[4], var[1], var[2], rw, mk)
            np.testing.assert_array_equal(rec['states'][t + 1], var[0])
            np.testing.assert_array_equal(rec['rm_host'][0, t], rw)
            np.testing.assert_array_equal(rec['rm_host'][1, t], mk)
    return gs, book.episodes


@pytest.mark.parametrize('arch,max_rep,nb', [('NIPS', 0, 1), ('NATURE', 10, 11), ('BAYESIAN', 0, 1)])
def test_learner_async_equals_lockstep(tmp_path, arch, max_rep, nb):
    """--runner device --sampling device, ec = 8, T = 5, lives 1, max_balls 3, 6 updates: the rollout
    enqueued without a host synchronisation == the same with one after every step, in every state slot,
    index, reward, mask, parameter and RMSProp slot; the device-written clipped rewards and masks == what
    the bookkeeping produced on the host; episode records and global_step == a host replay."""
    A = _learner(tmp_path / 'a', 'device', 'device', arch=arch, max_rep=max_rep, nb=nb)
    ta = _run(A, 6)
    fa = _final(A)
    gs, episodes = _host_replay(A, ta, 1, 3)
    A.cleanup()
    B = _learner(tmp_path / 'b', 'device', 'device', arch=arch, max_rep=max_rep, nb=nb, lockstep=True)
    tb = _run(B, 6)
    fb = _final(B)
    B.cleanup()
    for u, (x, y) in enumerate(zip(ta, tb)):
        for k in ('states', 'idx', 'rm_dev', 'rm_host'):
            np.testing.assert_array_equal(x[k], y[k], err_msg='%s update %d' % (k, u))
        np.testing.assert_array_equal(x['rm_dev'], x['rm_host'], err_msg='device vs bookkeeping, update %d' % u)
    for k in ('params', 'ms', 'mom'):
        np.testing.assert_array_equal(fa[k], fb[k], err_msg=k)
    assert fa['gs'] == fb['gs'] == gs == 6 * 5 * 8
    assert fa['episodes'] == fb['episodes'] and len(fa['episodes']) > 0
    assert [(int(g), float(r), int(n)) for g, r, n in fa['episodes']] == [(int(g), float(r), int(n))
                                                                           for g, r, n in episodes]


LEARN_BUDGET = 8192  # updates: twice the slowest of three measured seeds (4096; DESIGN.md "Catch")


def test_it_learns(tmp_path):
    """NIPS, ec 32, T 5, the pretrained/catcher hyper-parameters, seed 0, --runner device --sampling device
    (deterministic: counter-based draws, no float atomics). The bar is a definition: the mean return of
    the last 100 finished episodes reaches the midpoint between the uniform-random policy's mean return
    over 100 episodes (host restatement, nothing rendered) and max_balls, which tests/test_catch_cpu.py
    shows attainable. Measured with tools/catch_learn.py: seeds 0 / 1 / 2 first reach it after 3888 /
    3158 / 4096 updates (under 2 s each); the budget is twice the largest."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import catch_learn
    lives, max_balls = 3, 20
    cfg, st = catch.config(lives, max_balls), _lib.mt_catch_state()
    catch.host_reset(cfg, 0, 0, 1, st)
    rs, tab, rets, ret = np.random.RandomState(12345), np.zeros(1, np.int32), [], 0.0
    while len(rets) < 100:
        rw, over, _ = catch.host_step(cfg, 0, 0, 1, tab, int(rs.randint(3)), 0, st)
        ret += rw
        if over:
            rets.append(ret)
            ret = 0.0
    random_mean = float(np.mean(rets))
    assert -lives <= random_mean < 0
    target = 0.5 * (random_mean + max_balls)
    L = catch_learn.make_learner(str(tmp_path), 0, ec=32, lives=lives, max_balls=max_balls)
    try:
        updates, reached, curve = catch_learn.train_until(L, target, LEARN_BUDGET, every=1000)
    finally:
        L.cleanup()
    print('random %.3f  bar %.3f  updates %d  curve %s' % (random_mean, target, updates, curve))
    assert reached, (target, curve)


def test_device_runner_equals_python_runner(tmp_path):
    """--runner device --sampling host == --runner python --sampling host (CatchEmulator through the
    reference-contract runner): the same game under the same numpy stream, states and parameters after
    4 updates, bit for bit."""
    A = _learner(tmp_path / 'a', 'device', 'host', max_rep=10, nb=11)
    ta = _run(A, 4)
    fa = _final(A)
    A.cleanup()
    B = _learner(tmp_path / 'b', 'python', 'host', max_rep=10, nb=11)
    tb = _run(B, 4)
    fb = _final(B)
    B.cleanup()
    for u, (x, y) in enumerate(zip(ta, tb)):
        for k in ('states', 'idx', 'rm_host'):
            np.testing.assert_array_equal(x[k], y[k], err_msg='%s update %d' % (k, u))
    for k in ('params', 'ms', 'mom'):
        np.testing.assert_array_equal(fa[k], fb[k], err_msg=k)
    assert fa['gs'] == fb['gs'] and fa['episodes'] == fb['episodes'] and len(fa['episodes']) > 0
