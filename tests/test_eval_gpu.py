"""Device evaluation on the GPU: the three kernels against their host restatements bit for bit (in a
guarded arena), DeviceEvaluator against the games' host faces (recorded indices replayed on CatchEmulator /
BricksEmulator), determinism (same seed, graph against eager, BAYESIAN, LSTM), the macro-step cap, a
trained policy against its initial parameters on the identical games, training bit-identical with and
without --eval_every, and the two command lines."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_ref
import test_eval_cpu as cpu
from manette_amd import _lib, evaluate
from manette_amd.network import _ptr
from scratch_util import Arena

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- kernels against host --------------------------------------------------------------------------
class DeviceEval(object):
    """An eval state and the step inputs carved out of one sentinel arena."""

    def __init__(self, N, K, R):
        self.N, self.K, self.R = N, K, R
        sizes = dict(ret_acc=4 * N, len_acc=8 * N, done=4 * N, returns=4 * N * K, lengths=8 * N * K, words=16,
                     summary=56, r_idx=4 * N, reward=4 * N, over=4 * N, tab=4 * R)
        self.arena = Arena(sizes)
        b = self.arena.buf
        self.t = dict(ret_acc=b('ret_acc', torch.float32), len_acc=b('len_acc', torch.int64), done=b('done', torch.int32),
                      returns=b('returns', torch.float32), lengths=b('lengths', torch.int64),
                      words=b('words', torch.int64), summary=b('summary'), r_idx=b('r_idx', torch.int32),
                      reward=b('reward', torch.float32), over=b('over', torch.float32), tab=b('tab', torch.int32))
        a = lambda k: self.t[k].data_ptr()
        self.state = _lib.mt_eval_state(a('ret_acc'), a('len_acc'), a('done'), a('returns'), a('lengths'), a('words'),
                                        N, K)
        self.t['tab'].copy_(torch.from_numpy(eval_ref.TABS[R]))
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def reset(self):
        _lib.check(_lib.hip().mt_eval_reset(C.byref(self.state), self.stream), 'mt_eval_reset')

    def step(self, r_idx, reward, over):
        for k, v in (('r_idx', r_idx), ('reward', reward), ('over', over)):
            self.t[k].copy_(torch.from_numpy(v))
        _lib.check(_lib.hip().mt_eval_step(C.byref(self.state), _ptr(self.t['r_idx']), _ptr(self.t['reward']),
                                           _ptr(self.t['over']), _ptr(self.t['tab']), self.R, self.stream),
                   'mt_eval_step')

    def summarize(self):
        _lib.check(_lib.hip().mt_eval_summarize(C.byref(self.state), _ptr(self.t['summary']), self.stream),
                   'mt_eval_summarize')
        return self.t['summary'].cpu().numpy().tobytes()

    def fetch(self):
        """The buffers as host arrays under HostEval's names."""
        g = lambda k: self.t[k].cpu().numpy()
        self.ret_acc, self.len_acc, self.done = g('ret_acc'), g('len_acc'), g('done')
        self.returns, self.lengths = g('returns').reshape(self.N, self.K), g('lengths').reshape(self.N, self.K)
        self.words = g('words')
        return self


class _AsRef(object):
    """A HostEval seen through the reference's field names (assert_state_equal's second argument)."""

    def __init__(self, h):
        self.ret_acc, self.len_acc, self.done, self.returns, self.lengths = (h.ret_acc, h.len_acc, h.done, h.returns,
                                                                             h.lengths)
        self.remaining, self.steps = int(h.words[0]), int(h.words[1])


@pytest.mark.parametrize('N,K,R', eval_ref.GRID)
def test_kernels_equal_host_restatement(N, K, R):
    tab = eval_ref.TABS[R]
    d, h = DeviceEval(N, K, R), cpu.HostEval(N, K)
    for mode in eval_ref.OVER_MODES:
        d.reset()
        h.reset()
        cpu.assert_state_equal(d.fetch(), _AsRef(h), '%s after reset' % mode)
        for t, (r_idx, reward, over) in enumerate(eval_ref.sequence(N, K, R, mode)):
            d.step(r_idx, reward, over)
            h.step(r_idx, reward, over, tab)
            if t in eval_ref.SUMMARY_AT:
                where = '%s step %d' % (mode, t)
                cpu.assert_state_equal(d.fetch(), _AsRef(h), where)
                got = d.summarize()
                h.summarize()
                assert got == bytes(h.summary), where
    d.arena.check()


# ---- the evaluator -----------------------------------------------------------------------------------
def _setup(game, arch, rgb=False, max_rep=0, nb=1, seed=0, egreedy=False, **cfg):
    """(network with random initial parameters, env creator, tab_rep, args) as test.py builds them."""
    sys.path.insert(0, ROOT)
    import train as cli
    from manette_amd.exploration_policy import ExplorationPolicy
    a = cli.get_arg_parser().parse_args([])
    a.game, a.arch, a.rgb, a.max_repetition, a.nb_choices, a.seed, a.egreedy = game, arch, rgb, max_rep, nb, seed, egreedy
    for k, v in cfg.items():
        setattr(a, k, v)
    explo = ExplorationPolicy(a)
    nc, creator = cli.get_network_and_environment_creator(a, explo)
    net = nc()
    net.init_params(seed + 1)
    return net, creator, explo.tab_rep, a


def _replay(creator, tab_rep, trace, N, K):
    """The recorded indices played on the host faces, env by env: (returns [N][K], lengths [N][K], done [N]).
    An env is left alone once its K episodes are done (the later steps of a frozen env are ignored)."""
    returns, lengths, done = np.zeros((N, K), np.float32), np.zeros((N, K), np.int64), np.zeros(N, np.int32)
    for e in range(N):
        emu = creator.create_environment(e)
        emu.get_initial_state()
        ret, ln = np.float32(0), 0
        for step in trace:
            if done[e] == K:
                break
            a, r = int(step[0, e]), int(step[1, e])
            total, over = 0.0, False
            for _ in range(tab_rep[r] + 1):
                _, rw, over = emu.next(a)
                total += rw
                if over:
                    break
            ret = np.float32(ret + np.float32(total))
            ln += tab_rep[r] + 1
            if over:
                returns[e, done[e]], lengths[e, done[e]] = ret, ln
                done[e] += 1
                ret, ln = np.float32(0), 0
                emu.get_initial_state()
    return returns, lengths, done


@pytest.mark.parametrize('game,arch,rgb,max_rep,nb,cfg', [
    ('catch', 'NIPS', False, 0, 1, dict(catch_lives=2, catch_max_balls=4)),
    ('bricks', 'NATURE', True, 10, 11, dict(bricks_lives=2, bricks_max_nexts=60, bricks_serve_wait=2))])
def test_evaluator_equals_host_faces(game, arch, rgb, max_rep, nb, cfg):
    N, K = 5, 2
    net, creator, tab_rep, _ = _setup(game, arch, rgb, max_rep, nb, **cfg)
    ev = evaluate.DeviceEvaluator(net, creator, tab_rep, N, episodes=K, draw_seed=7, env0=0, check_every=6, record=True)
    res = ev.run()
    ev.close()
    assert res.unfinished == 0 and res.episodes == N * K and (res.done == K).all()
    assert res.trace.shape == (res.macro_steps, 2, N) and res.macro_steps % 6 == 0
    returns, lengths, done = _replay(creator, tab_rep, res.trace, N, K)
    np.testing.assert_array_equal(done, res.done)
    np.testing.assert_array_equal(returns.view(np.uint32), res.returns.view(np.uint32))
    np.testing.assert_array_equal(lengths, res.lengths)
    fin = res.returns.astype(np.float64).reshape(-1)
    assert abs(res.mean - fin.mean()) <= 1e-12 * max(1.0, np.abs(fin).mean())
    assert abs(res.std - fin.std()) <= 1e-9 * max(1.0, fin.std())
    assert res.min == fin.min() and res.max == fin.max() and res.mean_length == lengths.mean()
    if nb > 1:
        assert len(set(res.trace[:, 1].reshape(-1).tolist())) > 1  # the repetition head was used


def _tables(res):
    return res.returns.view(np.uint32).copy(), res.lengths.copy(), res.done.copy(), res.macro_steps


def _assert_same(a, b, what):
    for x, y, name in zip(_tables(a), _tables(b), ('returns', 'lengths', 'done', 'macro_steps')):
        np.testing.assert_array_equal(x, y, err_msg='%s: %s' % (what, name))


def test_same_seed_twice_and_graph_equals_eager():
    net, creator, tab_rep, _ = _setup('catch', 'NIPS', catch_lives=2, catch_max_balls=4)
    kw = dict(episodes=2, draw_seed=3, env0=0, check_every=4)
    g = evaluate.DeviceEvaluator(net, creator, tab_rep, 9, graph=True, **kw)
    e = evaluate.DeviceEvaluator(net, creator, tab_rep, 9, graph=False, **kw)
    first = g.run()
    assert g._graph is not None and first.macro_steps >= 12  # one eager block, one captured, replays
    again = g.run()                                           # replays from the first block on
    eager = e.run()
    assert e._graph is None
    _assert_same(first, again, 'the same seed twice')
    _assert_same(first, eager, 'graph against eager')
    other = evaluate.DeviceEvaluator(net, creator, tab_rep, 9, graph=False, **dict(kw, draw_seed=4)).run()
    assert not np.array_equal(other.returns, first.returns) or not np.array_equal(other.lengths, first.lengths)
    g.close()
    assert first.unfinished == 0 and first.episodes == 18


def test_check_every_is_rounded_up_to_even():
    net, creator, tab_rep, _ = _setup('catch', 'NIPS', catch_lives=1, catch_max_balls=2)
    a = evaluate.DeviceEvaluator(net, creator, tab_rep, 3, check_every=5, draw_seed=1, env0=0)
    b = evaluate.DeviceEvaluator(net, creator, tab_rep, 3, check_every=6, draw_seed=1, env0=0, graph=False)
    assert a.check_every == 6
    _assert_same(a.run(), b.run(), 'check_every 5 -> 6')
    a.close()


@pytest.mark.parametrize('arch', ['BAYESIAN', 'LSTM'])
def test_bayesian_and_lstm_run_and_are_deterministic(arch):
    net, creator, tab_rep, _ = _setup('catch', arch, catch_lives=1, catch_max_balls=3)
    train_ws = None
    if arch == 'BAYESIAN':  # a training workspace's dropout state must not move
        net.set_dropout_state('rollout', 99, 5, batch=3)
        train_ws = net.dropout_state(net.workspace(3, 'rollout'), 3)
    g = evaluate.DeviceEvaluator(net, creator, tab_rep, 3, draw_seed=5, env0=0, check_every=4, graph=True)
    e = evaluate.DeviceEvaluator(net, creator, tab_rep, 3, draw_seed=5, env0=0, check_every=4, graph=False)
    first, again, eager = g.run(), g.run(), e.run()
    g.close()
    assert first.unfinished == 0 and first.episodes == 3
    _assert_same(first, again, arch + ' twice')
    _assert_same(first, eager, arch + ' graph against eager')
    if train_ws is not None:
        now = net.dropout_state(net.workspace(3, 'rollout'), 3)
        assert now[:2] == train_ws[:2] and np.array_equal(now[2], train_ws[2])
        seed, row0, counters = net.dropout_state(net.workspace(3, 'eval'), 3)
        assert (counters == eager.macro_steps).all()  # dropout stayed on: one mask per row and forward


def test_max_macro_steps_caps_the_run():
    net, creator, tab_rep, _ = _setup('catch', 'NIPS')
    ev = evaluate.DeviceEvaluator(net, creator, tab_rep, 4, episodes=2, draw_seed=1, env0=0, max_macro_steps=3)
    res = ev.run()
    ev.close()
    assert res.macro_steps == 3 and res.unfinished > 0
    assert res.episodes == int(res.done.sum()) == 4 * 2 - res.unfinished
    assert res.episodes == 0 and res.mean == 0.0 and res.std == 0.0  # (no Catch episode ends within 3 steps)


def test_default_cap_comes_from_the_game():
    from manette_amd import bricks, catch
    net, creator, tab_rep, _ = _setup('catch', 'NIPS', catch_max_balls=7)
    ev = evaluate.DeviceEvaluator(net, creator, tab_rep, 2, episodes=3)
    assert ev.max_macro_steps == 3 * catch.max_episode_nexts(catch.config(3, 7)) + 1
    netb, creatorb, tabb, _ = _setup('bricks', 'NIPS', bricks_max_nexts=33)
    evb = evaluate.DeviceEvaluator(netb, creatorb, tabb, 2, episodes=2)
    assert evb.max_macro_steps == 2 * 33 + 1 == 2 * bricks.max_episode_nexts(evb.env.cfg) + 1


def test_it_tells_a_trained_policy_from_its_initial_parameters(tmp_path):
    """tests/test_catch_gpu.py::test_it_learns's recipe and seed (NIPS, ec 32, seed 0, trained to that
    test's bar within its budget), then 64 envs under the argmax chooser, once with the initial and once
    with the trained parameters, on the identical games. Measured ("Device evaluation"): mean
    return -2.30 with the initial parameters, 11.77 after the 3888 updates that reach the bar. No absolute
    bar is fixed here, the training bar being a statement about sampled training episodes."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import catch_learn
    from test_catch_gpu import LEARN_BUDGET
    lives, max_balls = 3, 20
    target = catch_learn.bar(lives, max_balls)
    L = catch_learn.make_learner(str(tmp_path), 0, ec=32, lives=lives, max_balls=max_balls)
    try:
        argmax = evaluate.policy_from_args(None, greedy=True)
        ev = evaluate.DeviceEvaluator(L.network, L.environment_creator, L.tab_rep, 64, policy=argmax, draw_seed=1,
                                      env0=evaluate.EVAL_ENV0)
        initial = ev.run()
        updates, reached, _ = catch_learn.train_until(L, target, LEARN_BUDGET)
        assert reached
        trained = ev.run()
        ev.close()
    finally:
        L.cleanup()
    print('updates %d  initial %r  trained %r' % (updates, initial, trained))
    assert initial.episodes == trained.episodes == 64 and initial.unfinished == trained.unfinished == 0
    assert trained.mean > initial.mean, (trained.mean, initial.mean)


# ---- training untouched ------------------------------------------------------------------------------
EC, T = 8, 5


def _learner(tmp, graph, eval_every):
    sys.path.insert(0, ROOT)
    import train as cli
    from manette_amd.exploration_policy import ExplorationPolicy
    from manette_amd.paac import PAACLearner
    a = cli.get_arg_parser().parse_args([])
    a.game, a.arch, a.emulator_counts, a.emulator_workers = 'catch', 'NIPS', EC, 0
    a.runner, a.sampling, a.seed = 'device', 'device', 0
    a.catch_lives, a.catch_max_balls = 1, 3
    a.iteration_graph, a.drain_every = graph, 3
    a.eval_every, a.eval_envs, a.eval_episodes = eval_every, 6, 2
    a.debugging_folder = str(tmp) + '/'
    a.max_global_steps = 6 * T * EC
    a.checkpoint_interval = 1 << 40
    a.lr_annealing_steps = 100000
    cli.validate_args(a)
    np.random.seed(1234)
    explo = ExplorationPolicy(a)
    nc, ec_ = cli.get_network_and_environment_creator(a, explo)
    return PAACLearner(nc, ec_, explo, a)


def _final(L):
    g = lambda x: x.cpu().numpy().copy()
    return dict(params=g(L.network.params), ms=g(L.network.ms), mom=g(L.network.mom), states=g(L.states),
                idx=g(L.idx), counters=g(L.counters), env=g(L.env.state), gs=L.global_step,
                episodes=list(L.book.episodes))


@pytest.mark.parametrize('graph', [False, True])
def test_training_is_bit_identical_with_evaluation(tmp_path, graph):
    from manette_amd import summary
    out = {}
    for name, every in (('plain', 0), ('eval', 2 * T * EC)):
        L = _learner(tmp_path / name, graph, every)
        L.train()  # (cleanup keeps the device buffers)
        out[name] = (_final(L), L.eval_history)
    plain, ev = out['plain'][0], out['eval'][0]
    for k in ('params', 'ms', 'mom', 'states', 'idx', 'counters', 'env'):
        np.testing.assert_array_equal(ev[k], plain[k], err_msg=k)
    assert ev['gs'] == plain['gs'] == 6 * T * EC
    assert ev['episodes'] == plain['episodes'] and len(plain['episodes']) > 0
    assert out['plain'][1] == []
    steps = [s for s, _ in out['eval'][1]]
    # eager: after updates 2, 4 and 6; graph, drained every 3: at the first drain past each multiple
    assert steps == ([3 * T * EC, 6 * T * EC] if graph else [2 * T * EC, 4 * T * EC, 6 * T * EC])
    for _, res in out['eval'][1]:
        assert res.episodes == 12 and res.unfinished == 0
    def eval_tags(folder):
        d, tags = os.path.join(str(folder), 'tf'), {}
        for f in os.listdir(d):
            for _, step, vals in summary.read_events(os.path.join(d, f)):
                for tag, v in vals.items():
                    if tag.startswith('eval/'):
                        tags.setdefault(tag, []).append((step, v))
        return tags

    tags = eval_tags(tmp_path / 'eval')
    assert sorted(tags) == sorted(summary.EVAL_TAGS)
    assert [s for s, _ in tags['eval/mean_return']] == steps
    last = out['eval'][1][-1][1]
    assert tags['eval/mean_return'][-1][1] == np.float32(last.mean)
    assert eval_tags(tmp_path / 'plain') == {}


# ---- the command lines -------------------------------------------------------------------------------
def test_cli_train_then_test_on_the_device(tmp_path):
    df = str(tmp_path / 'run') + '/'
    env = dict(os.environ, PYTHONPATH=ROOT)
    tr = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '-g', 'catch', '--runner', 'device',
                         '--sampling', 'device', '--arch', 'NIPS', '-ec', '8', '-ew', '0', '--max_global_steps', '320',
                         '--catch_lives', '1', '--catch_max_balls', '3', '--eval_every', '160', '--eval_envs', '4',
                         '-df', df], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert tr.returncode == 0, tr.stdout[-2000:] + tr.stderr[-2000:]
    assert len(re.findall(r'Evaluation at step \d+', tr.stdout + tr.stderr)) == 2
    outs = []
    for _ in range(2):
        ev = subprocess.run([sys.executable, os.path.join(ROOT, 'test.py'), '-f', df, '-tc', '4', '--runner', 'device',
                             '--greedy', '--draw_seed', '1'], cwd=ROOT, env=env, capture_output=True, text=True,
                            timeout=300)
        assert ev.returncode == 0, ev.stdout[-2000:] + ev.stderr[-2000:]
        lines = [l for l in ev.stdout.splitlines() if re.match(r'(Performed|Mean:|Min:|Max:|Std:)', l)]
        assert len(lines) == 5 and lines[0] == 'Performed 4 tests for catch.', ev.stdout
        for l in lines[1:]:
            assert re.match(r'(Mean|Min|Max|Std): -?\d+\.\d\d$', l), l
        assert '-np is not applied' in ev.stderr
        outs.append(lines)
    assert outs[0] == outs[1]
