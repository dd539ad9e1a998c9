"""Device exploration policy on the GPU (include/manette_hip.h, mt_policy): mt_sample_policy and the
draw fused into the heads kernel against the host restatement mt_policy_draw_host, the zero policy
against mt_sample, and the learner (native macro-step == Python step) under annealed e-greedy.

The fused draw has no rollout-free entry point, so it is pinned through the learner's native
macro-step (mt_rollout_step): every recorded (a, r) against mt_policy_draw_host on the pi / rep the
heads kernel wrote."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import policy_ref as ref
from policy_ref import ARGMAX, EGREEDY

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5eed1234abcd


def _sample(pol, pi, rep, ctr, row0, seed=SEED):
    from manette_amd.network import sample
    B = pi.shape[0]
    a = torch.full((B,), -1, dtype=torch.int32, device='cuda')
    r = torch.full((B,), -1, dtype=torch.int32, device='cuda')
    pair = torch.full((2, B), -1, dtype=torch.int32, device='cuda')
    sample(pi, rep, seed, ctr, a, r, pair=pair, row0=row0, policy=pol)
    a, r, pair = a.cpu().numpy(), r.cpu().numpy(), pair.cpu().numpy()
    np.testing.assert_array_equal(pair[0], a)
    np.testing.assert_array_equal(pair[1], r)
    return a, r


def _rows(rs, n, B):
    rows = rs.dirichlet(np.ones(n), size=B).astype(np.float32)
    for k, (_, row, _) in enumerate(ref.special_rows(n)):  # tie, last, NaN, all-equal — and in the ragged tail
        rows[k] = row
        rows[B - 1 - k] = row
    return rows


@pytest.mark.parametrize('row0', [0, 8])
@pytest.mark.parametrize('name', ['egreedy', 'annealed', 'argmax'])
def test_sample_policy_equals_host(name, row0):
    """B = 70 (more than one 64-thread block, ragged tail), A = 18, R = 11, 10 successive calls (the
    annealed policy — rows_per_call 8, annealing_steps 56 — crosses zero at call 7): every index equals
    mt_policy_draw_host, counters advance by one per call."""
    pol = dict(egreedy=ref.policy(EGREEDY, 0.3), annealed=ref.policy(EGREEDY, 0.3, True, 56.0, 8),
               argmax=ref.policy(ARGMAX))[name]
    B, A, R = 70, 18, 11
    rs = np.random.RandomState(17)
    pi_h, rep_h = _rows(rs, A, B), _rows(rs, R, B)[::-1].copy()
    pi, rep = torch.from_numpy(pi_h).cuda(), torch.from_numpy(rep_h).cuda()
    ctr = torch.zeros(B, dtype=torch.int64, device='cuda')
    explored = []
    for call in range(10):
        a, r = _sample(pol, pi, rep, ctr, row0)
        assert (ctr.cpu().numpy() == call + 1).all()
        want = [ref.host_draw(pol, SEED, row0 + b, call, pi_h[b], rep_h[b]) for b in range(B)]
        np.testing.assert_array_equal(a, [w[0] for w in want], err_msg='action, call %d' % call)
        np.testing.assert_array_equal(r, [w[1] for w in want], err_msg='repetition, call %d' % call)
        greedy = np.array([np.argmax(pi_h[b]) for b in range(B)])
        explored.append(int((a != greedy).sum()))
    if name == 'egreedy':
        assert all(explored)
    if name == 'annealed':
        assert explored[0] > 0 and not any(explored[7:])
    if name == 'argmax':
        assert not any(explored)


def test_zero_policy_is_mt_sample():
    """A zero-filled policy through mt_sample_policy is bit-identical to mt_sample on the same inputs
    and counters (B = 70, both heads, 6 calls, row0 = 8)."""
    B, A, R = 70, 18, 11
    rs = np.random.RandomState(23)
    pi = torch.from_numpy(rs.dirichlet(np.ones(A), size=B).astype(np.float32)).cuda()
    rep = torch.from_numpy(rs.dirichlet(np.ones(R), size=B).astype(np.float32)).cuda()
    c0 = torch.zeros(B, dtype=torch.int64, device='cuda')
    c1 = torch.zeros(B, dtype=torch.int64, device='cuda')
    zero = ref.policy()
    assert bytes(zero) == bytes(C.sizeof(zero))
    for _ in range(6):
        a0, r0 = _sample(None, pi, rep, c0, 8)
        a1, r1 = _sample(zero, pi, rep, c1, 8)
        np.testing.assert_array_equal(a0, a1)
        np.testing.assert_array_equal(r0, r1)
        np.testing.assert_array_equal(c0.cpu().numpy(), c1.cpu().numpy())
    assert len(np.unique(a0)) > 1 and len(np.unique(r0)) > 1


# ---- the learner ---------------------------------------------------------------------------------

def _learner(tmp, arch='NIPS', ec=8, game='pong', max_rep=0, nb=1, t_max=5, staging='resized', pipeline=True,
             egreedy=True, epsilon=0.3, annealed=True, annealed_steps=96, test=False):
    sys.path.insert(0, ROOT)
    import train as cli
    from manette_amd.exploration_policy import ExplorationPolicy
    from manette_amd.paac import PAACLearner
    a = cli.get_arg_parser().parse_args([])
    a.game, a.arch, a.emulator_counts, a.emulator_workers = game, arch, ec, 2
    a.max_repetition, a.nb_choices, a.max_local_steps = max_rep, nb, t_max
    a.runner, a.sampling, a.seed, a.staging, a.pipeline = 'native', 'device', 0, staging, pipeline
    a.egreedy, a.epsilon, a.annealed, a.annealed_steps = egreedy, epsilon, annealed, annealed_steps
    a.keep_percentage = 0.8
    a.debugging_folder = str(tmp) + '/'
    a.max_global_steps = 1 << 40
    a.checkpoint_interval = 1 << 40
    a.lr_annealing_steps = 100000
    np.random.seed(1234)
    explo = ExplorationPolicy(a, test=test)
    nc, ec_ = cli.get_network_and_environment_creator(a, explo)
    L = PAACLearner(nc, ec_, explo, a)  # (before the device policy: ValueError for egreedy + device)
    L.start()
    return L


def _run(L, updates):
    """`updates` rollouts + updates; per rollout the index arrays and the pi / rep the draw read."""
    rec = []
    T = L.max_local_steps
    for _ in range(updates):
        L.book.new_update()
        for t in range(T):
            L.step(t)
        L.update()
        torch.cuda.synchronize()
        c = lambda x: x.cpu().numpy().copy()
        rec.append(dict(a=c(L.a_idx), r=c(L.r_idx), pi=c(L.pi_all[:T]), rep=c(L.rep_all[:T])))
    return rec


def _check_against_host(L, rec):
    """Every recorded (a, r) == mt_policy_draw_host(policy, sample_seed, env_offset + e, n T + t, the
    recorded pi / rep). Returns per call (explored rows, epsilon) for the action head."""
    T, E = L.max_local_steps, L.emulator_counts
    calls = []
    for n, roll in enumerate(rec):
        for t in range(T):
            call = n * T + t
            eps = ref.epsilon_of(L.policy, call)
            explored = 0
            for e in range(E):
                pi, rep = roll['pi'][t, e], roll['rep'][t, e]
                want = ref.host_draw(L.policy, L.sample_seed, L.env_offset + e, call, pi, rep)
                assert (int(roll['a'][t, e]), int(roll['r'][t, e])) == want, (n, t, e)
                explored += float(ref.uniforms(L.sample_seed, L.env_offset + e, call)[0]) < eps
                if eps == 0.0:
                    assert want == (int(np.argmax(pi)), int(np.argmax(rep)))
            calls.append((explored, eps))
    return calls


def _python_step(L):
    from manette_amd import _lib
    _lib.hip().mt_rollout_destroy(L.native_step)
    L.native_step = None
    return L


def _final(L):
    return dict(params=L.network.params.cpu().numpy().copy(), ms=L.network.ms.cpu().numpy().copy(), gs=L.global_step)


@pytest.mark.parametrize('arch,game,nb,A', [('NIPS', 'pong', 1, 6), ('NATURE', 'seaquest', 11, 18)])
def test_fused_draw_equals_host(tmp_path, arch, game, nb, A):
    """The heads kernel's draw at E = 5: NIPS A = 6, R = 1 (4 waves) and NATURE A = 18, R = 11 (8 waves,
    F = 512), constant epsilon 0.3, two rollouts (the second from the replayed rollout graph)."""
    L = _learner(tmp_path, arch=arch, ec=5, game=game, max_rep=10 if nb > 1 else 0, nb=nb, annealed=False)
    try:
        assert L.native_step is not None and L.num_actions == A and L.policy.mode == EGREEDY
        rec = _run(L, 2)
        calls = _check_against_host(L, rec)
        assert sum(x for x, _ in calls) > 0 and all(eps == 0.3 for _, eps in calls)
        if nb == 1:
            assert not any(r['r'].any() for r in rec)
    finally:
        L.cleanup()


@pytest.mark.parametrize('max_rep,nb', [(0, 1), (10, 11)])
def test_native_step_equals_python_step_egreedy(tmp_path, max_rep, nb):
    """NIPS, ec = 8, t_max = 5, --egreedy --epsilon 0.3 --annealed --annealed_steps 96, 4 updates = 20
    draw calls per row: epsilon reaches 0 at call 12, the later rollouts replay the rollout graph with
    epsilon 0. The native macro-step (pipelined stacking chains, fused draw) and the Python step
    (mt_sample_policy) give identical index arrays and parameters; every native (a, r) equals the host
    restatement; explored and greedy choices both occur before call 12, only the argmax from call 12."""
    A = _learner(tmp_path / 'a', max_rep=max_rep, nb=nb)
    try:
        assert A.native_step is not None
        ra = _run(A, 4)
        calls = _check_against_host(A, ra)
        fa = _final(A)
    finally:
        A.cleanup()
    B = _python_step(_learner(tmp_path / 'b', max_rep=max_rep, nb=nb, staging='copy', pipeline=False))
    try:
        rb = _run(B, 4)
        fb = _final(B)
    finally:
        B.cleanup()
    for n, (x, y) in enumerate(zip(ra, rb)):
        for k in ('a', 'r', 'pi', 'rep'):
            np.testing.assert_array_equal(x[k], y[k], err_msg='%s of rollout %d' % (k, n))
    for k in ('params', 'ms'):
        np.testing.assert_array_equal(fa[k], fb[k], err_msg=k)
    assert fa['gs'] == fb['gs'] == 4 * 5 * 8
    assert len(calls) == 20
    before = calls[:12]
    explored, rows = sum(x for x, _ in before), 8 * len(before)
    print('explore share before call 12: %d / %d = %.4f, mean epsilon %.4f'
          % (explored, rows, explored / rows, np.mean([eps for _, eps in before])))
    assert 0 < explored < rows
    assert all(eps > 0 for _, eps in calls[:12]) and all(eps == 0.0 and x == 0 for x, eps in calls[12:])


def test_lstm_native_step_equals_host(tmp_path):
    """LSTM (lstm_step_forward hands the same SampleArgs to the heads kernel), ec = 4, t_max = 2, FiGAR
    heads, 2 updates, annealed over 12 global steps: calls 0..2 explore with epsilon > 0, call 3 on 0."""
    L = _learner(tmp_path, arch='LSTM', ec=4, t_max=2, max_rep=10, nb=11, annealed_steps=12, epsilon=0.9)
    try:
        assert L.native_step is not None
        calls = _check_against_host(L, _run(L, 2))
        assert [eps > 0 for _, eps in calls] == [True, True, True, False]
    finally:
        L.cleanup()


def test_bayesian_python_step_equals_host(tmp_path):
    """BAYESIAN has no native macro-step: its Python step draws with mt_sample_policy. ec = 4, t_max = 2,
    constant epsilon 0.5, one update."""
    L = _learner(tmp_path, arch='BAYESIAN', ec=4, t_max=2, annealed=False, epsilon=0.5)
    try:
        assert L.native_step is None and L.policy.mode == EGREEDY
        calls = _check_against_host(L, _run(L, 1))
        assert len(calls) == 2
    finally:
        L.cleanup()


def test_test_policy_is_argmax_on_the_device(tmp_path):
    """ExplorationPolicy(test=True) maps to ARGMAX: every native choice is the first maximum."""
    L = _learner(tmp_path, ec=4, t_max=2, egreedy=False, test=True)
    try:
        assert L.native_step is not None and L.policy.mode == ARGMAX
        rec = _run(L, 1)
        _check_against_host(L, rec)
        np.testing.assert_array_equal(rec[0]['a'], rec[0]['pi'].argmax(axis=2))
    finally:
        L.cleanup()


def test_set_policy_is_refused_after_the_first_step(tmp_path):
    from manette_amd import _lib
    lib = _lib.hip()
    L = _learner(tmp_path, ec=4, t_max=2, egreedy=False)
    try:
        assert L.native_step is not None and L.policy is None
        pol = ref.policy(EGREEDY, 0.1)
        bad = ref.policy(EGREEDY, 1.5)
        assert lib.mt_rollout_set_policy(L.native_step, C.byref(bad)) == 1 and b'epsilon' in lib.mt_last_error()
        assert lib.mt_rollout_set_policy(L.native_step, C.byref(pol)) == 0
        assert lib.mt_rollout_set_policy(L.native_step, None) == 0  # back to the multinomial draw
        L.book.new_update()
        L.step(0)
        assert lib.mt_rollout_set_policy(L.native_step, C.byref(pol)) == 1
        assert b'first mt_rollout_step' in lib.mt_last_error()
        L.step(1)
        L.update()
        torch.cuda.synchronize()
    finally:
        L.cleanup()
