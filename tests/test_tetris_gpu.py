"""Tetris on the GPU, test for test as tests/test_bricks_gpu.py at its shapes: the env kernel (mt_tetris_step:
step, render and stack in one launch) against the host restatement bit for bit (random play, a start wait,
and every crafted state with the rewards recorded from the reference's own code), its fused stack against the
existing stacking kernel, poisoned outputs inside a sentinel arena, launch splits, graph capture, argument
checks, the learner's device runner against its lockstep form, its replayed-graph form and the
reference-contract Python runner, device evaluation against the host faces, and that it learns."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import scratch_util
import tetris_cases
import tetris_ref
from manette_amd import _lib, tetris

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = tetris_cases.SEED  # (the crafted cases' draws were recorded at this seed)
TABS = {1: [0], 11: list(range(11))}
FAST = (6, 1, 0)  # (max_nexts, speed, max_start_wait): an episode ends within a few macro-steps
DEFAULT = (2000, 5, 0)
CONFIGS = [FAST, DEFAULT]
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'tetris_rule.npz')
OUT_KEYS = ('reward', 'over', 'clipped', 'mask', 'state', 'obs')


class Rig(object):
    """A TetrisDevice with its buffers; step(a, r) plays one macro-step prev -> out and swaps them."""

    def __init__(self, E, R, depth=1, cfg=DEFAULT, env0=0, T=3, frames=True):
        self.E, self.R, self.depth, self.env0, self.T, self.t = E, R, depth, env0, T, 0
        self.dev = tetris.TetrisDevice(E, TABS[R], seed=SEED, env0=env0, rgb=depth == 3, max_nexts=cfg[0],
                                       speed=cfg[1], max_start_wait=cfg[2])
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

    def set_actions(self, a, r):
        self.a.copy_(torch.as_tensor(np.asarray(a, np.int32)))
        self.r.copy_(torch.as_tensor(np.asarray(r, np.int32)))

    def launch(self, t=None):
        self.dev.step(self.a, self.r, self.bufs[0], self.bufs[1], self.reward, self.over, self.rm,
                      self.t if t is None else t, self.T, self.frames, self.count)

    def step(self, a, r):
        self.set_actions(a, r)
        self.launch()
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
    """The same envs on mt_tetris_*_host."""

    def __init__(self, E, R, depth=1, cfg=DEFAULT, env0=0):
        self.E, self.depth, self.env0 = E, depth, env0
        self.tab = np.asarray(TABS[R], np.int32)
        self.cfg = tetris.config(*cfg)
        self.st = [_lib.mt_tetris_state() for _ in range(E)]
        self.obs = np.zeros((E, 84, 84, 4 * depth), np.uint8)
        for e in range(E):
            tetris.host_reset(self.cfg, SEED, env0 + e, depth, self.st[e], self.obs[e])

    def step(self, a, r):
        E = self.E
        out = np.empty_like(self.obs)
        res = dict(reward=np.zeros(E, np.float32), over=np.zeros(E, np.float32), count=np.zeros(E, np.int32),
                   frames=np.zeros((4 * E, 84, 84, self.depth), np.uint8))
        for e in range(E):
            rw, ov, cnt = tetris.host_step(self.cfg, SEED, self.env0 + e, self.depth, self.tab, a[e], r[e], self.st[e],
                                           self.obs[e], out[e], res['frames'][4 * e:4 * e + 4])
            res['reward'][e], res['over'][e], res['count'][e] = rw, ov, cnt
        self.obs = out
        res.update(obs=out, clipped=np.clip(res['reward'], -1, 1), mask=1 - res['over'],
                   state=np.frombuffer(b''.join(bytes(s) for s in self.st), dtype=tetris.STATE_DTYPE))
        return res


def _actions(step, E, R, wild=False):
    ar = [tetris_ref.hashed_actions(step, e, R) for e in range(E)]
    a, r = [x for x, _ in ar], [y for _, y in ar]
    if wild:  # out-of-range indices: clamped in the kernel as on the host
        a[0], r[0], a[1], r[1] = -3, -7, 11, 10 ** 6
    return a, r


def _assert_same(got, want, frames=True, where=''):
    for k in OUT_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg='%s %s' % (k, where))
    if frames:
        np.testing.assert_array_equal(got['count'], want['count'], err_msg='count ' + where)
        for e, c in enumerate(want['count']):  # (slots past the count are not written)
            np.testing.assert_array_equal(got['frames'][4 * e:4 * e + c], want['frames'][4 * e:4 * e + c],
                                          err_msg='frames env %d %s' % (e, where))


@pytest.mark.parametrize('env0', [0, 37])
@pytest.mark.parametrize('cfg', CONFIGS)
@pytest.mark.parametrize('R', [1, 11])
@pytest.mark.parametrize('depth', [1, 3])
def test_kernel_matches_host(depth, R, cfg, env0):
    """Every output of mt_tetris_step, 25 macro-steps of E = 5 envs, bit for bit."""
    d = Rig(5, R, depth, cfg, env0)
    h = HostRig(5, R, depth, cfg, env0)
    np.testing.assert_array_equal(d.obs.cpu().numpy(), h.obs)
    np.testing.assert_array_equal(d.dev.state_array(), np.frombuffer(b''.join(bytes(s) for s in h.st),
                                                                     dtype=tetris.STATE_DTYPE))
    ended = 0
    for step in range(25):
        a, r = _actions(step, 5, R, wild=step % 7 == 3)
        t = d.step(a, r)
        want = h.step(a, r)
        _assert_same(d.outputs(t), want, where='step %d' % step)
        ended += int(want['over'].sum())
    if cfg == FAST:
        assert ended > 0


def test_kernel_matches_host_64_envs():
    d, h = Rig(64, 11, 1, FAST), HostRig(64, 11, 1, FAST)
    for step in range(2):
        a, r = _actions(step, 64, 11)
        t = d.step(a, r)
        _assert_same(d.outputs(t), h.step(a, r), where='step %d' % step)


def test_kernel_matches_host_with_start_wait():
    """max_start_wait 30 under a cap of 6 nexts at speed 1: every few macro-steps a new game whose w + 4 initial
    acts (w drawn per game) are played inside the kernel; RGB, R = 11, env0 = 37."""
    cfg = (6, 1, 30)
    d, h = Rig(5, 11, 3, cfg, 37), HostRig(5, 11, 3, cfg, 37)
    np.testing.assert_array_equal(d.obs.cpu().numpy(), h.obs)
    ended, counters = 0, set()
    for step in range(12):
        a, r = _actions(step, 5, 11)
        t = d.step(a, r)
        want = h.step(a, r)
        _assert_same(d.outputs(t), want, where='step %d' % step)
        ended += int(want['over'].sum())
        counters |= set(want['state']['speed_counter'][want['over'] != 0].tolist())
    assert ended > 5 and len(counters) > 3  # (a new game's speed_counter is w + 4)


@pytest.mark.parametrize('depth', [1, 3])
def test_crafted_states_in_one_batch(depth):
    """Every crafted state of tests/tetris_cases.py as one batch (env e = case e), two macro-steps from random
    previous stacks: device == host in every output, and the first step's rewards and episode ends are what
    the fixture recorded from the reference's own act()."""
    cases = tetris_cases.CASES
    gold = np.load(GOLDEN)
    E = len(cases)
    kw = dict(E=E, R=1, depth=depth, cfg=DEFAULT, env0=tetris_cases.ENV)
    d, h = Rig(**kw), HostRig(**kw)
    rec = np.zeros(E, dtype=tetris.STATE_DTYPE)
    for e, (_, state, _) in enumerate(cases):
        rec[e] = tetris_ref.state_tuple(**state)
        tetris_ref.fill_state(h.st[e], **state)
    assert rec.tobytes() == b''.join(bytes(x) for x in h.st)
    d.dev.state.copy_(torch.from_numpy(rec.view(np.uint8).reshape(E, -1).copy()))
    prev = np.random.RandomState(3).randint(0, 256, h.obs.shape).astype(np.uint8)
    h.obs = prev.copy()
    d.bufs[0].copy_(torch.from_numpy(prev))
    a = [c[2] for c in cases]
    for step in range(2):
        t = d.step(a, [0] * E)
        want = h.step(a, [0] * E)
        got = d.outputs(t)
        _assert_same(got, want, where='step %d' % step)
        if step == 0:
            np.testing.assert_array_equal(got['reward'], gold['case_reward'].astype(np.float32))
            np.testing.assert_array_equal(got['over'], gold['case_gameover'].astype(np.float32))


@pytest.mark.parametrize('depth', [1, 3])
def test_fused_stack_equals_preprocess_resized(depth):
    """The kernel's render-and-stack pass == mt_preprocess_resized on its frames_out / push_count_out and
    the same prev (table 0..10: pushes from 1 to more than 4, and resets)."""
    from manette_amd import network as devnet
    E = 5
    d = Rig(E, 11, depth, FAST)
    off = torch.arange(0, 4 * E, 4, dtype=torch.int32, device='cuda')
    for step in range(12):
        a, r = _actions(step, E, 11)
        prev = d.obs
        d.step(a, r)
        want = torch.zeros_like(prev)
        devnet.preprocess(d.frames, off, d.count, E, depth, None, None, prev, want, resized=True)
        np.testing.assert_array_equal(d.obs.cpu().numpy(), want.cpu().numpy(), err_msg='step %d' % step)


@pytest.mark.parametrize('E', [1, 5, 33])
@pytest.mark.parametrize('pattern', ['nan', 'stale'])
def test_outputs_are_written_not_accumulated_and_confined(E, pattern):
    """Every output pre-filled with NaN words or stale floats and carved at its exact size inside a sentinel
    arena (guards before, between and after): three macro-steps give the clean run's bits (frames up to the
    push count) and leave the guards intact. The rm rows that the call does not write keep their fill."""
    depth, T, R = 3, 3, 11
    clean = Rig(E, R, depth, FAST, T=T)
    sizes = dict(state=E * tetris.STATE_BYTES, prev=E * 84 * 84 * 4 * depth, out=E * 84 * 84 * 4 * depth,
                 frames=4 * E * 84 * 84 * depth, count=4 * E, reward=4 * E, over=4 * E, rm=4 * 2 * T * E, a=4 * E, r=4 * E)
    arena = scratch_util.Arena(sizes)
    rig = Rig(E, R, depth, FAST, T=T)
    rig.dev.state = arena.buf('state').view(E, tetris.STATE_BYTES)
    rig.bufs = [arena.buf('prev').view(E, 84, 84, 4 * depth), arena.buf('out').view(E, 84, 84, 4 * depth)]
    rig.frames = arena.buf('frames').view(4 * E, 84, 84, depth)
    rig.count, rig.a, rig.r = (arena.buf(k, torch.int32) for k in ('count', 'a', 'r'))
    rig.reward, rig.over = arena.buf('reward', torch.float32), arena.buf('over', torch.float32)
    rig.rm = arena.buf('rm', torch.float32).view(2, T, E)
    rig.dev.reset(rig.bufs[0])
    rs = np.random.RandomState(5)
    for step in range(3):
        a, r = _actions(step, E, R)
        for name in ('reward', 'over', 'rm', 'count'):
            scratch_util.fill(arena.buf(name, torch.int32), pattern, rs)
        scratch_util.fill(rig.bufs[1].reshape(-1).view(torch.int32), pattern, rs)
        scratch_util.fill(rig.frames.reshape(-1).view(torch.int32), pattern, rs)
        rm_before = rig.rm.view(torch.int32).cpu().numpy().copy()
        t = rig.step(a, r)
        tc = clean.step(a, r)
        got, want = rig.outputs(t), clean.outputs(tc)
        _assert_same(got, want, where='step %d' % step)
        rm_after = rig.rm.view(torch.int32).cpu().numpy()
        for row in range(T):
            if row != t:
                np.testing.assert_array_equal(rm_after[:, row], rm_before[:, row])
        arena.check()


def test_launch_split():
    """E = 8 in one launch == two launches with env0 = 0 (3 envs) and env0 = 3 (5 envs)."""
    cfg = FAST
    whole = Rig(8, 11, 1, cfg, frames=False)
    parts = [(0, 3, Rig(3, 11, 1, cfg, env0=0, frames=False)), (3, 8, Rig(5, 11, 1, cfg, env0=3, frames=False))]
    for step in range(12):
        a, r = _actions(step, 8, 11)
        got = whole.outputs(whole.step(a, r))
        for lo, hi, p in parts:
            want = p.outputs(p.step(a[lo:hi], r[lo:hi]))
            for k in OUT_KEYS:
                np.testing.assert_array_equal(got[k][lo:hi], want[k], err_msg='%s step %d' % (k, step))


def test_capture_and_replay():
    """One captured mt_tetris_step replayed 3 times == 3 eager calls: the state advances in device memory
    and the indices are read at replay time, nothing is baked into the graph."""
    lib = _lib.hip()
    g_rig, e_rig = Rig(5, 11, 1, FAST), Rig(5, 11, 1, FAST)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sp = C.c_void_p(side.cuda_stream)
        _lib.check(lib.mt_graph_begin(sp), 'mt_graph_begin')
        g_rig.launch(0)
        graph = C.c_void_p()
        _lib.check(lib.mt_graph_end(sp, C.byref(graph)), 'mt_graph_end')
    try:
        last = None
        for k in range(3):
            a, r = _actions(k, 5, 11)
            a[2], r[2] = 3, 10  # env 2: 11 nexts per replay, so its game ends (the cap is 6) in every one
            g_rig.set_actions(a, r)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                _lib.check(lib.mt_graph_launch(graph, C.c_void_p(side.cuda_stream)), 'mt_graph_launch')
            side.synchronize()
            got = dict(obs=g_rig.bufs[1].cpu().numpy(), state=g_rig.dev.state_array().copy(),
                       reward=g_rig.reward.cpu().numpy(), over=g_rig.over.cpu().numpy())
            e_rig.set_actions(a, r)
            e_rig.launch(0)
            torch.cuda.synchronize()
            want = dict(obs=e_rig.bufs[1].cpu().numpy(), state=e_rig.dev.state_array().copy(),
                        reward=e_rig.reward.cpu().numpy(), over=e_rig.over.cpu().numpy())
            for key in want:
                np.testing.assert_array_equal(got[key], want[key], err_msg='%s replay %d' % (key, k))
            assert want['over'][2] == 1
            if last is not None:
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
    torch.cuda.synchronize()
    before = d.outputs(0)
    bads = [(3, 0), (4, 2), (6, 0), (17, 3), (17, -1), (18, 0), (2, -1), (11, p(d.bufs[0])), (9, None), (16, None),
            (5, None), (12, p(d.frames)), (13, p(d.count)), (11, C.c_void_p(d.bufs[1].data_ptr() + 4)),
            (10, C.c_void_p(d.bufs[0].data_ptr() + 8)), (9, C.c_void_p(d.dev.state.data_ptr() + 4)),
            (0, C.byref(tetris.config(0, 5, 0))), (0, C.byref(tetris.config(5, 0, 0))),
            (0, C.byref(tetris.config(5, 5, -1))), (0, C.byref(tetris.config(5, 5, 31))), (0, None)]
    for i, v in bads:
        bad = list(base)
        bad[i] = v
        assert lib.mt_tetris_step(*bad) == 1, i
    rbase = [C.byref(d.dev.cfg), C.c_uint64(1), 0, 4, 1, p(d.dev.state), p(d.bufs[1]), None]
    for i, v in ((3, 0), (2, -1), (4, 4), (5, None), (6, None), (6, C.c_void_p(d.bufs[1].data_ptr() + 4))):
        bad = list(rbase)
        bad[i] = v
        assert lib.mt_tetris_reset(*bad) == 1, i
    torch.cuda.synchronize()
    after = d.outputs(0)
    for k in OUT_KEYS:  # nothing was launched
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    assert lib.mt_tetris_step(*base) == 0
    torch.cuda.synchronize()


# ---- the learner ---------------------------------------------------------------------------------
EC, T = 8, 5


def _learner(tmp, runner='device', sampling='device', arch='NIPS', max_rep=0, nb=1, rgb=False, lockstep=False,
             graph=False, cfg=FAST):
    sys.path.insert(0, ROOT)
    import train as cli
    from manette_amd.exploration_policy import ExplorationPolicy
    from manette_amd.paac import PAACLearner
    a = cli.get_arg_parser().parse_args([])
    a.game, a.arch, a.emulator_counts, a.emulator_workers = 'tetris', arch, EC, 0
    a.max_repetition, a.nb_choices, a.rgb = max_rep, nb, rgb
    a.runner, a.sampling, a.seed = runner, sampling, 0
    a.tetris_max_nexts, a.tetris_speed, a.random_start = cfg[0], cfg[1], cfg[2] == 30
    a.iteration_graph, a.drain_every = graph, 3 if graph else None
    a.debugging_folder = str(tmp) + '/'
    a.max_global_steps = 1 << 40
    a.checkpoint_interval = 1 << 40
    a.lr_annealing_steps = 100000
    np.random.seed(1234)
    explo = ExplorationPolicy(a)
    nc, ec_ = cli.get_network_and_environment_creator(a, explo)
    L = PAACLearner(nc, ec_, explo, a)
    assert L.max_local_steps == T and L.num_actions == 5
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
    torch.cuda.synchronize()
    g = lambda x: x.cpu().numpy().copy()
    return dict(params=g(L.network.params), ms=g(L.network.ms), mom=g(L.network.mom), states=g(L.states),
                idx=g(L.idx), gs=L.global_step, episodes=list(L.book.episodes),
                total_rewards=list(L.book.total_rewards), total_steps=list(L.book.total_steps))


@pytest.mark.parametrize('arch,max_rep,nb', [('NIPS', 0, 1), ('NATURE', 10, 11)])
def test_learner_async_equals_lockstep(tmp_path, arch, max_rep, nb):
    """--runner device --sampling device, ec = 8, T = 5, the fast config, 4 updates: the rollout enqueued
    without a host synchronisation == the same with one after every step, in every state slot, index,
    reward, mask, parameter and RMSProp slot; the device-written clipped rewards and masks == what the
    bookkeeping produced on the host."""
    A = _learner(tmp_path / 'a', arch=arch, max_rep=max_rep, nb=nb)
    ta, fa = _run(A, 4), None
    fa = _final(A)
    A.cleanup()
    B = _learner(tmp_path / 'b', arch=arch, max_rep=max_rep, nb=nb, lockstep=True)
    tb = _run(B, 4)
    fb = _final(B)
    B.cleanup()
    for u, (x, y) in enumerate(zip(ta, tb)):
        for k in ('states', 'idx', 'rm_dev', 'rm_host'):
            np.testing.assert_array_equal(x[k], y[k], err_msg='%s update %d' % (k, u))
        np.testing.assert_array_equal(x['rm_dev'], x['rm_host'], err_msg='device vs bookkeeping, update %d' % u)
    for k in ('params', 'ms', 'mom'):
        np.testing.assert_array_equal(fa[k], fb[k], err_msg=k)
    assert fa['gs'] == fb['gs'] == 4 * T * EC
    assert fa['episodes'] == fb['episodes'] and len(fa['episodes']) > 0


@pytest.mark.parametrize('arch,max_rep,nb,rgb', [('NATURE', 10, 11, False), ('PWYX', 0, 1, True)])
def test_iteration_graph_equals_eager(tmp_path, arch, max_rep, nb, rgb):
    """7 updates, drain_every 3 (one eager iteration, one capture, five replays) against the asynchronous
    eager path at the same seed: params, RMSProp slots, states, indices, global_step, episode records and
    the LR word. NATURE + FiGAR at A = 5, R = 11 is the second benchmark configuration on a real game."""
    ref = _learner(tmp_path / 'a', arch=arch, max_rep=max_rep, nb=nb, rgb=rgb)
    for _ in range(7):
        ref.book.new_update()
        ref.rollout()
        ref.update()
    want = _final(ref)
    want_lr = np.float32(ref.get_lr())
    ref.cleanup()
    L = _learner(tmp_path / 'b', arch=arch, max_rep=max_rep, nb=nb, rgb=rgb, graph=True)
    for u in range(7):
        L.book.new_update()
        L.rollout()
        lr = L.update()
        if (u + 1) % 3 == 0 or u == 6:
            assert L.drain() == (u + 1) * T * EC
    assert L._iter_graph is not None and L._iterations == 7
    got = _final(L)
    lr_word = L.book.lr_value
    L.cleanup()
    for k in ('params', 'ms', 'mom', 'states', 'idx'):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got['gs'] == want['gs'] == 7 * T * EC
    for k in ('episodes', 'total_rewards', 'total_steps'):
        assert got[k] == want[k] and len(want[k]) > 0, k
    assert np.float32(lr) == want_lr and lr_word.view(np.uint32) == want_lr.view(np.uint32)


LEARN_BUDGET = 210  # updates: twice the slowest of three measured seeds (105; DESIGN.md "Tetris")


def test_it_learns(tmp_path):
    """NIPS, ec 32, T 5, Catch's hyper-parameters unchanged (lr 0.02 annealed over 3e8 steps, entropy 0.02,
    clip 3, gamma 0.99), the default config, seed 0, --runner device --sampling device --iteration_graph
    drained after every update (deterministic: counter-based draws, no float atomics). Under clipped rewards
    the first thing to learn is that dropping pays, so the bar is on the reward per next(): the mean of return /
    length over the last 100 finished episodes. The bar is a definition: the midpoint between the
    uniform-random policy's value and the always-drop policy's, both over 100 episodes of the host
    restatement (numpy seed 12345, nothing rendered): 0.202 and 1.0, so 0.601. Measured with tools/catch_learn.py
    --game tetris --iteration_graph: seeds 0 / 1 / 2 first reach it after 104 / 100 / 105 updates (the first
    update at which 100 episodes have finished: by then the policy drops, at 0.88 per next); the budget is twice
    the largest. ec and the config are not lowered: the run takes well under a second."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import catch_learn
    rs = np.random.RandomState(12345)
    random_rate = catch_learn.tetris_policy_rate(lambda: int(rs.randint(5)), 100)
    drop_rate = catch_learn.tetris_policy_rate(lambda: 3, 100)
    assert 0 < random_rate < drop_rate
    target = 0.5 * (random_rate + drop_rate)
    assert target == catch_learn.tetris_bar()  # the tool's curves were measured against this bar
    L = catch_learn.make_learner(str(tmp_path), 0, ec=32, game='tetris', iteration_graph=True, drain_every=1)
    try:
        updates, reached, curve = catch_learn.train_until(L, target, LEARN_BUDGET, every=500, per_next=True)
    finally:
        L.cleanup()
    print('random %.3f  drop %.3f  bar %.3f  updates %d  curve %s' % (random_rate, drop_rate, target, updates, curve))
    assert reached, (target, curve)


def test_device_runner_equals_python_runner(tmp_path):
    """--runner device --sampling host == --runner python --sampling host (TetrisEmulator through the
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


def test_device_evaluation_equals_host_faces():
    """DeviceEvaluator on Tetris (NATURE + FiGAR R = 11, RGB, a cap of 60 nexts at speed 2): the recorded indices
    replayed on the host faces give the same returns, lengths and episode counts (tests/test_eval_gpu.py's form)."""
    from manette_amd import evaluate
    from test_eval_gpu import _replay, _setup
    N, K = 5, 2
    net, creator, tab_rep, _ = _setup('tetris', 'NATURE', True, 10, 11, tetris_max_nexts=60, tetris_speed=2)
    ev = evaluate.DeviceEvaluator(net, creator, tab_rep, N, episodes=K, draw_seed=7, env0=0, check_every=6, record=True)
    assert ev.max_macro_steps == 2 * 60 + 1
    res = ev.run()
    ev.close()
    assert res.unfinished == 0 and res.episodes == N * K and (res.done == K).all()
    returns, lengths, done = _replay(creator, tab_rep, res.trace, N, K)
    np.testing.assert_array_equal(done, res.done)
    np.testing.assert_array_equal(returns.view(np.uint32), res.returns.view(np.uint32))
    np.testing.assert_array_equal(lengths, res.lengths)
    assert len(set(res.trace[:, 1].reshape(-1).tolist())) > 1 and res.returns.max() > 0
