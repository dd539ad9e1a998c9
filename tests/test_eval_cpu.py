"""Device evaluation without a GPU: the host restatements mt_eval_*_host against the numpy restatement
(tests/eval_ref.py) bit for bit, the summary against float64 numpy, the empty summary, every refusal,
the games' max_episode_nexts bounds, and the new flags of train.py / test.py."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import eval_ref
from manette_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY_FIELDS = ('episodes', 'unfinished', 'length_sum', 'sum', 'sumsq', 'min', 'max')


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class HostEval(object):
    """An eval state in host memory driven through mt_eval_*_host (every buffer starts as garbage)."""

    def __init__(self, N, K):
        self.N, self.K = N, K
        self.ret_acc = np.full(N, 9.0, np.float32)
        self.len_acc = np.full(N, 9, np.int64)
        self.done = np.full(N, 9, np.int32)
        self.returns = np.full((N, K), 9.0, np.float32)
        self.lengths = np.full((N, K), 9, np.int64)
        self.words = np.full(2, 9, np.int64)
        self.summary = _lib.mt_eval_summary()
        self.state = _lib.mt_eval_state(_p(self.ret_acc), _p(self.len_acc), _p(self.done), _p(self.returns),
                                        _p(self.lengths), _p(self.words), N, K)

    def reset(self):
        _lib.check(_lib.hip().mt_eval_reset_host(C.byref(self.state)), 'mt_eval_reset_host')

    def step(self, r_idx, reward, over, tab_rep):
        _lib.check(_lib.hip().mt_eval_step_host(C.byref(self.state), _p(r_idx), _p(reward), _p(over), _p(tab_rep),
                                                len(tab_rep)), 'mt_eval_step_host')

    def summarize(self):
        _lib.check(_lib.hip().mt_eval_summarize_host(C.byref(self.state), C.byref(self.summary)),
                   'mt_eval_summarize_host')
        s = self.summary
        assert s.pad[0] == 0 and s.pad[1] == 0
        return dict(episodes=s.episodes, unfinished=s.unfinished, length_sum=s.length_sum, sum=s.sum, sumsq=s.sumsq,
                    min=np.float32(s.min), max=np.float32(s.max))


def assert_state_equal(h, ref, where):
    """Every buffer and both words, bit for bit (h: anything with HostEval's arrays)."""
    np.testing.assert_array_equal(h.ret_acc.view(np.uint32), ref.ret_acc.view(np.uint32), err_msg='ret_acc ' + where)
    np.testing.assert_array_equal(h.len_acc, ref.len_acc, err_msg='len_acc ' + where)
    np.testing.assert_array_equal(h.done, ref.done, err_msg='done ' + where)
    np.testing.assert_array_equal(h.returns.view(np.uint32), ref.returns.view(np.uint32), err_msg='returns ' + where)
    np.testing.assert_array_equal(h.lengths, ref.lengths, err_msg='lengths ' + where)
    assert (int(h.words[0]), int(h.words[1])) == (ref.remaining, ref.steps), where


def assert_summary_equal(got, want, where):
    for k in SUMMARY_FIELDS:
        g, w = got[k], want[k]
        if k in ('sum', 'sumsq'):
            g, w = np.float64(g).view(np.uint64), np.float64(w).view(np.uint64)
        elif k in ('min', 'max'):
            g, w = np.float32(g).view(np.uint32), np.float32(w).view(np.uint32)
        assert g == w, (k, got[k], want[k], where)


def assert_summary_close_to_numpy(got, ref, where):
    """Against float64 numpy on the finished entries of the table: 1e-12 relative."""
    fin = ref.returns[np.arange(ref.K)[None, :] < ref.done[:, None]].astype(np.float64)
    assert got['episodes'] == fin.size and got['unfinished'] == ref.remaining, where
    assert got['length_sum'] == int(ref.lengths[np.arange(ref.K)[None, :] < ref.done[:, None]].sum()), where
    if fin.size == 0:
        for k in SUMMARY_FIELDS:
            if k != 'unfinished':
                assert got[k] == 0, (k, where)
        return
    for k, want in (('sum', fin.sum()), ('sumsq', (fin * fin).sum())):
        assert abs(got[k] - want) <= 1e-12 * max(abs(want), np.abs(fin).sum() if k == 'sum' else want), (k, where)
    assert got['min'] == np.float32(fin.min()) and got['max'] == np.float32(fin.max()), where


@pytest.mark.parametrize('mode', eval_ref.OVER_MODES)
@pytest.mark.parametrize('N,K,R', eval_ref.GRID)
def test_host_equals_numpy_restatement(N, K, R, mode):
    tab = eval_ref.TABS[R]
    h, ref = HostEval(N, K), eval_ref.EvalRef(N, K)
    h.reset()
    ref.reset()
    assert_state_equal(h, ref, 'after reset')
    for t, (r_idx, reward, over) in enumerate(eval_ref.sequence(N, K, R, mode)):
        h.step(r_idx, reward, over, tab)
        ref.step(r_idx, reward, over, tab)
        assert_state_equal(h, ref, 'step %d' % t)
        if t in eval_ref.SUMMARY_AT:
            got = h.summarize()
            assert_summary_equal(got, ref.summarize(), 'step %d' % t)
            assert_summary_close_to_numpy(got, ref, 'step %d' % t)
    if mode == 'ones':  # every env froze after K steps: the later steps left nothing
        assert ref.remaining == 0 and (ref.done == K).all() and (ref.lengths > 0).all()
    elif mode == 'zeros':
        assert ref.remaining == N * K and ref.summarize()['episodes'] == 0
    # a second reset starts over from a used state
    h.reset()
    ref.reset()
    assert_state_equal(h, ref, 'second reset')


def test_sequences_freeze_early_and_leave_unfinished():
    """What the random sequences are for: at the early summaries some envs are frozen, some still play."""
    N, K, R = 1000, 1, 11
    ref = eval_ref.EvalRef(N, K)
    ref.reset()
    for t, (r_idx, reward, over) in enumerate(eval_ref.sequence(N, K, R, 'random')):
        ref.step(r_idx, reward, over, eval_ref.TABS[R])
        if t == 4:
            assert 0 < ref.remaining < N * K
    assert ref.steps == eval_ref.STEPS


def test_length_counts_planned_nexts_under_the_clamps():
    """tab_rep entries beyond [0, 255] and r_idx outside [0, R) are clamped as the env kernels clamp."""
    tab = eval_ref.TABS[11]
    h = HostEval(4, 1)
    h.reset()
    r = np.array([-5, 6, 7, 99], np.int32)  # -> entries 0, 300, -4, 12 -> nexts 1, 256, 1, 13
    z = np.zeros(4, np.float32)
    h.step(r, z, z, tab)
    np.testing.assert_array_equal(h.len_acc, [1, 256, 1, 13])
    h.step(r, np.ones(4, np.float32), np.ones(4, np.float32), tab)
    np.testing.assert_array_equal(h.lengths[:, 0], [2, 512, 2, 26])
    np.testing.assert_array_equal(h.returns[:, 0], [1, 1, 1, 1])
    h.step(r, np.ones(4, np.float32), np.ones(4, np.float32), tab)  # frozen
    np.testing.assert_array_equal(h.lengths[:, 0], [2, 512, 2, 26])
    np.testing.assert_array_equal(h.len_acc, [0, 0, 0, 0])
    assert list(h.words) == [0, 3]


def test_empty_summary():
    h = HostEval(7, 2)
    h.reset()
    h.returns[...] = 5.0  # not counted: done is 0 everywhere
    got = h.summarize()
    assert got == dict(episodes=0, unfinished=14, length_sum=0, sum=0.0, sumsq=0.0, min=np.float32(0), max=np.float32(0))


def _refused(rc):
    assert rc != 0
    assert _lib.hip().mt_last_error()


@pytest.mark.parametrize('device', [False, True])
def test_refusals(device):
    """MT_ERR_ARG before any launch (the device entry points are refused on host pointers without a GPU:
    nothing is launched, nothing dereferenced)."""
    lib = _lib.hip()
    h = HostEval(8, 2)
    h.reset()
    tab = eval_ref.TABS[11]
    r, f = np.zeros(8, np.int32), np.zeros(8, np.float32)

    def reset(st):
        return lib.mt_eval_reset(C.byref(st), None) if device else lib.mt_eval_reset_host(C.byref(st))

    def step(st, r_idx=_p(r), reward=_p(f), over=_p(f), tab_rep=_p(tab), R=11):
        if device:
            return lib.mt_eval_step(C.byref(st), r_idx, reward, over, tab_rep, R, None)
        return lib.mt_eval_step_host(C.byref(st), r_idx, reward, over, tab_rep, R)

    def summarize(st, out):
        return lib.mt_eval_summarize(C.byref(st), out, None) if device else lib.mt_eval_summarize_host(C.byref(st), out)

    def variant(**kw):
        st = _lib.mt_eval_state()
        C.memmove(C.byref(st), C.byref(h.state), C.sizeof(st))
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    out = C.cast(C.byref(h.summary), C.c_void_p)
    bad_states = [variant(**{k: None}) for k in ('ret_acc', 'len_acc', 'done', 'returns', 'lengths', 'words')]
    bad_states += [variant(N=0), variant(K=0), variant(N=-3), variant(N=1 << 20, K=(1 << 10) + 1)]
    bad_states += [variant(**{k: getattr(h.state, k) + 4}) for k in ('len_acc', 'lengths', 'words')]
    for st in bad_states:
        _refused(reset(st))
        _refused(step(st))
        _refused(summarize(st, out))
    for kw in (dict(r_idx=None), dict(reward=None), dict(over=None), dict(tab_rep=None), dict(R=0), dict(R=-1)):
        _refused(step(h.state, **kw))
    _refused(summarize(h.state, None))
    _refused(summarize(h.state, C.c_void_p(out.value + 4)))
    if device:
        _refused(lib.mt_eval_reset(None, None))
    else:
        _refused(lib.mt_eval_reset_host(None))
        # nothing was touched by any refused call; N * K = 2^30 exactly is within the limit's wording
        ref = eval_ref.EvalRef(8, 2)
        ref.reset()
        assert_state_equal(h, ref, 'after the refusals')


# ---- the games' bounds -------------------------------------------------------------------------------
def _episode_nexts(mod, cfg, env, policy_rs, episodes):
    """The next() counts of `episodes` consecutive episodes of one env under random (or noop) play."""
    state = (_lib.mt_catch_state if mod.__name__.endswith('catch') else _lib.mt_bricks_state)()
    one = np.zeros(1, np.int32)
    mod.host_reset(cfg, 3, env, 1, state)
    out, n = [], 0
    while len(out) < episodes:
        a = 0 if policy_rs is None else int(policy_rs.randint(0, mod.NUM_ACTIONS))
        _, over, _ = mod.host_step(cfg, 3, env, 1, one, a, 0, state)
        n += 1
        if over:
            out.append(n)
            n = 0
    return out


@pytest.mark.parametrize('game', ['catch', 'bricks'])
@pytest.mark.parametrize('small', [False, True])
def test_max_episode_nexts_bounds_host_play(game, small):
    import importlib
    mod = importlib.import_module('manette_amd.' + game)
    if game == 'catch':
        cfg = mod.config(1, 3) if small else mod.config()
    else:
        cfg = mod.config(1, 40, 2) if small else mod.config()
    bound = mod.max_episode_nexts(cfg)
    assert bound >= 1
    for env, rs in ((0, np.random.RandomState(11)), (5, None)):
        nexts = _episode_nexts(mod, cfg, env, rs, 50)
        assert len(nexts) == 50 and max(nexts) <= bound, (max(nexts), bound)


# ---- flags -------------------------------------------------------------------------------------------
def _train_args(argv):
    sys.path.insert(0, ROOT)
    import train as cli
    return cli, cli.get_arg_parser().parse_args(argv)


def load_test_cli():
    """The repository's test.py as a module (by path: `test` is also a standard-library package)."""
    import importlib.util
    sys.path.insert(0, ROOT)
    spec = importlib.util.spec_from_file_location('manette_test_cli', os.path.join(ROOT, 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_parser_defaults():
    _, a = _train_args([])
    assert (a.eval_every, a.eval_envs, a.eval_episodes, a.eval_greedy) == (0, 64, 1, False)


def test_validate_args_accepts_and_refuses():
    cli, _ = _train_args([])
    ok = [['-g', 'catch', '--runner', 'device', '--eval_every', '1000'],
          ['-g', 'bricks', '--runner', 'python', '--eval_every', '1000', '--eval_envs', '3', '--eval_episodes', '2',
           '--eval_greedy'],
          ['-g', 'catch', '--runner', 'device', '--sampling', 'device', '--iteration_graph', '--eval_every', '640'],
          ['-g', 'pong'], ['-g', 'pong', '--eval_envs', '5']]
    for argv in ok:
        cli.validate_args(cli.get_arg_parser().parse_args(argv))
    bad = [(['-g', 'pong', '--eval_every', '1000'], 'device environment'),
           (['-g', 'breakout', '--eval_greedy'], 'catch'),
           (['-g', 'catch', '--runner', 'device', '--eval_every', '-1'], 'eval_every'),
           (['-g', 'catch', '--runner', 'device', '--eval_every', '10', '--eval_envs', '0'], 'eval_envs'),
           (['-g', 'catch', '--runner', 'device', '--eval_every', '10', '--eval_episodes', '0'], 'eval_episodes')]
    for argv, word in bad:
        with pytest.raises(ValueError, match=word):
            cli.validate_args(cli.get_arg_parser().parse_args(argv))


def test_test_parser_defaults_and_named_error(tmp_path):
    test_cli = load_test_cli()
    a = test_cli.get_arg_parser().parse_args(['-f', str(tmp_path)])
    assert (a.test_runner, a.greedy, a.draw_seed, a.episodes_per_env) == ('host', False, None, 1)
    _, train_args = _train_args(['-g', 'pong'])
    with open(os.path.join(str(tmp_path), 'args.json'), 'w') as f:
        json.dump(vars(train_args), f)
    a = test_cli.get_arg_parser().parse_args(['-f', str(tmp_path), '--runner', 'device', '-tc', '4'])
    with pytest.raises(ValueError, match='catch.*bricks'):
        test_cli.run(a)


def test_eval_state_layout():
    from manette_amd import evaluate
    lay, total = evaluate.state_layout(5, 3)
    at = 0
    for name in ('words', 'summary', 'ret_acc', 'len_acc', 'done', 'returns', 'lengths'):
        off, n = lay[name]
        assert off >= at and off % 16 == 0
        at = off + n
    assert total >= at and lay['words'] == (0, 16)
    assert evaluate.EVAL_ENV0 == 1 << 20
