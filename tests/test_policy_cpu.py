"""Device exploration policy (include/manette_hip.h, mt_policy) without a GPU: the host restatement
mt_policy_draw_host against a numpy restatement of the rule written here (tests/policy_ref.py), the
argmax special rows, the epsilon edge values against ExplorationPolicy.get_epsilon, the e-greedy
distribution, the argument checks and the zero policy."""
import ctypes as C
import types

import numpy as np
import pytest

import policy_ref as ref
from policy_ref import ARGMAX, EGREEDY, MULTINOMIAL

SEED = 0x5eed1234abcd
SIZES = [(A, R) for A in (1, 6, 18, 32) for R in (1, 11, 31)]
assert all(1 + A + R <= 64 for A, R in SIZES)


def _policies():
    return [('multinomial', ref.policy()),
            ('egreedy', ref.policy(EGREEDY, 0.3)),
            ('egreedy_annealed', ref.policy(EGREEDY, 0.9, True, 56.0, 8)),
            ('argmax', ref.policy(ARGMAX))]


def _rows(rs, n, count):
    rows = [rs.dirichlet(np.ones(n)).astype(np.float32) for _ in range(count)]
    if n >= 3:
        rows += [row for _, row, _ in ref.special_rows(n)]
    return rows


def _chi2_ok(counts, probs, alpha=1e-4):
    from scipy.stats import chi2
    nz = probs > 0
    assert counts[~nz].sum() == 0, 'a zero-probability category was drawn'
    n = counts.sum()
    exp = probs[nz] * n
    stat = float(((counts[nz] - exp) ** 2 / exp).sum())
    pval = chi2.sf(stat, max(int(nz.sum()) - 1, 1))
    assert pval > alpha, (stat, pval, counts, exp)
    return pval


@pytest.mark.parametrize('A,R', SIZES)
def test_host_draw_equals_numpy_rule(A, R):
    """All three modes (e-greedy constant and annealed), 2,048 (row, counter) pairs each: random
    Dirichlet rows plus the tie / last / NaN / all-equal rows; rows and counters small and huge."""
    rs = np.random.RandomState(100 * A + R)
    pis, reps = _rows(rs, A, 12), _rows(rs, R, 12)
    rows = list(range(40)) + [2 ** 20 + 3, 2 ** 23 - 1]
    counters = list(range(44)) + [1000, 2 ** 40 + 7, 2 ** 52 + 1, 2 ** 63 + 5, 2 ** 64 - 1]
    pairs = [(r, c) for r in rows for c in counters]
    assert len(pairs) >= 2048
    for name, pol in _policies():
        explored = 0
        for k, (row, c) in enumerate(pairs):
            pi, rep = pis[k % len(pis)], reps[(k // 3) % len(reps)]
            got = ref.host_draw(pol, SEED, row, c, pi, rep)
            assert got == ref.draw(pol, SEED, row, c, pi, rep), (name, row, c)
            assert 0 <= got[0] < A and 0 <= got[1] < R
            if R == 1:
                assert got[1] == 0
            explored += float(ref.uniforms(SEED, row, c)[0]) < ref.epsilon_of(pol, c)
        if name == 'egreedy':
            assert 0.2 < explored / len(pairs) < 0.4
        if name in ('multinomial', 'argmax'):
            assert explored == 0


@pytest.mark.parametrize('n', [3, 6, 18, 32])
def test_argmax_special_rows(n):
    """Two equal maxima: the first; the maximum last; a NaN: the first NaN; all equal: index 0 — on
    both heads, under ARGMAX and under EGREEDY with epsilon 0."""
    for name, row, want in ref.special_rows(n):
        assert int(np.argmax(row)) == want, name
        for pol in (ref.policy(ARGMAX), ref.policy(EGREEDY, 0.0)):
            for c in range(16):
                assert ref.host_draw(pol, SEED, 3, c, row, row[::-1].copy()) == (want, int(np.argmax(row[::-1]))), name


def test_epsilon_zero_is_argmax_and_one_always_explores():
    rs = np.random.RandomState(5)
    A, R = 6, 11
    for row in range(24):
        for c in range(24):
            pi, rep = rs.dirichlet(np.ones(A)).astype(np.float32), rs.dirichlet(np.ones(R)).astype(np.float32)
            greedy = ref.host_draw(ref.policy(ARGMAX), SEED, row, c, pi, rep)
            assert greedy == (int(np.argmax(pi)), int(np.argmax(rep)))
            assert ref.host_draw(ref.policy(EGREEDY, 0.0), SEED, row, c, pi, rep) == greedy
            ua, ur = (float(x) for x in ref.uniforms(SEED, row, c))
            assert ref.host_draw(ref.policy(EGREEDY, 1.0), SEED, row, c, pi, rep) == (int(np.floor(ua * A)),
                                                                                      int(np.floor(ur * R)))


def test_annealed_epsilon_follows_the_exploration_policy():
    """rows_per_call = 8, annealing_steps = 56: counters 0..6 use eps0 (1 - c/7), counter 7 exactly 0
    (g == annealing_steps takes the first branch: eps0 - eps0), counters >= 8 use 0 — the rule's
    epsilon equals ExplorationPolicy.get_epsilon() at global_step = 8c, and the host draw follows it."""
    from manette_amd.exploration_policy import ExplorationPolicy
    eps0 = 0.3
    args = types.SimpleNamespace(egreedy=True, epsilon=eps0, softmax_temp=1.0, keep_percentage=1.0, annealed=True,
                                 annealed_steps=56, max_repetition=0, nb_choices=1)
    explo = ExplorationPolicy(args)
    pol = ref.policy(EGREEDY, eps0, True, 56.0, 8)
    rs = np.random.RandomState(11)
    A, R = 6, 11
    rows = [(rs.dirichlet(np.ones(A)).astype(np.float32), rs.dirichlet(np.ones(R)).astype(np.float32)) for _ in range(256)]
    for c in range(12):
        explo.global_step = 8 * c
        eps = ref.epsilon_of(pol, c)
        assert eps == explo.get_epsilon()
        if c < 7:
            assert eps == pytest.approx(eps0 * (1 - c / 7.0), rel=1e-12) and eps > 0
        else:
            assert eps == 0.0
        explored = 0
        for row, (pi, rep) in enumerate(rows):
            ua, ur = (float(x) for x in ref.uniforms(SEED, row, c))
            got = ref.host_draw(pol, SEED, row, c, pi, rep)
            assert got == (ref.choose_index(pi, ua, eps), ref.choose_index(rep, ur, eps))
            if c >= 7:
                assert got == ref.host_draw(ref.policy(ARGMAX), SEED, row, c, pi, rep)
            explored += ua < eps
        if c == 0:
            assert 0.2 * len(rows) < explored < 0.4 * len(rows)
        if c >= 7:
            assert explored == 0


def test_egreedy_distribution():
    """EGREEDY at eps = 0.3 over 32,768 host draws (128 rows x 256 counters, seed 20301, chosen on the
    CPU): the action head (A = 6) and the repetition head (R = 11) each against (1 - eps + eps/n) on
    the argmax and eps/n elsewhere, chi-square at alpha = 1e-4. Recorded p-values at this seed:
    action 0.5169, repetition 0.3945."""
    eps, A, R, seed = 0.3, 6, 11, 20301
    rs = np.random.RandomState(7)
    pi, rep = rs.dirichlet(np.ones(A)).astype(np.float32), rs.dirichlet(np.ones(R)).astype(np.float32)
    pol = ref.policy(EGREEDY, eps)
    ca, cr = np.zeros(A), np.zeros(R)
    for row in range(128):
        for c in range(256):
            a, r = ref.host_draw(pol, seed, row, c, pi, rep)
            ca[a] += 1
            cr[r] += 1
    assert ca.sum() == cr.sum() == 32768
    for counts, p, n in ((ca, pi, A), (cr, rep, R)):
        probs = np.full(n, eps / n)
        probs[int(np.argmax(p))] += 1 - eps
        print('p-value', _chi2_ok(counts, probs))


BAD = [('mode', dict(mode=3)), ('mode', dict(mode=-1)), ('epsilon', dict(mode=EGREEDY, epsilon=-0.01)),
       ('epsilon', dict(mode=EGREEDY, epsilon=1.01)), ('epsilon', dict(mode=EGREEDY, epsilon=float('nan'))),
       ('annealing_steps', dict(mode=EGREEDY, epsilon=0.1, annealed=True, annealing_steps=0.0)),
       ('annealing_steps', dict(mode=EGREEDY, epsilon=0.1, annealed=True, annealing_steps=-5.0)),
       ('annealing_steps', dict(mode=EGREEDY, epsilon=0.1, annealed=True, annealing_steps=float('nan'))),
       ('rows_per_call', dict(mode=EGREEDY, epsilon=0.1, rows_per_call=0)),
       ('rows_per_call', dict(mode=EGREEDY, epsilon=0.1, rows_per_call=-3))]


@pytest.mark.parametrize('field,kw', BAD)
def test_bad_policy_is_refused(field, kw):
    """MT_ERR_ARG with a message naming the field, from the host draw and from mt_sample_policy (which
    returns before any launch: its buffers are never touched, so host arrays stand in for them)."""
    from manette_amd import _lib
    lib = _lib.hip()
    pol = ref.policy(**kw)
    p = np.full(6, 1 / 6, np.float32)
    assert ref.host_draw(pol, 1, 0, 0, p, p, expect=1) == 1
    assert field.encode() in lib.mt_last_error()
    buf = np.zeros(64, np.int64)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert lib.mt_sample_policy(C.byref(pol), ptr, ptr, 2, 3, 3, 1, 0, ptr, ptr, ptr, None, None) == 1
    msg = lib.mt_last_error()
    assert msg and field.encode() in msg
    assert not buf.any()


def test_good_edge_policies_are_accepted():
    p = np.full(6, 1 / 6, np.float32)
    for kw in (dict(mode=EGREEDY, epsilon=0.0), dict(mode=EGREEDY, epsilon=1.0),
               dict(mode=EGREEDY, epsilon=0.5, annealing_steps=0.0),  # not annealed: the field is not read
               dict(mode=EGREEDY, epsilon=0.5, annealed=True, annealing_steps=1e-3)):
        a, r = ref.host_draw(ref.policy(**kw), 1, 0, 0, p, p)
        assert 0 <= a < 6 and 0 <= r < 6


def test_zero_and_null_policy_are_the_multinomial_draw():
    """A zero-filled policy and a NULL policy draw mt_sample's rule: the inverse CDF on (p - epsneg),
    the last category taking the remainder, for the same (seed, row, counter)."""
    rs = np.random.RandomState(2)
    A, R = 18, 11
    zero = ref.policy()
    assert bytes(zero) == bytes(C.sizeof(zero))
    for row in range(32):
        for c in range(32):
            pi, rep = rs.dirichlet(np.ones(A)).astype(np.float32), rs.dirichlet(np.ones(R)).astype(np.float32)
            ua, ur = (float(x) for x in ref.uniforms(SEED, row, c))
            want = (ref.multinomial_index(pi, ua), ref.multinomial_index(rep, ur))
            assert ref.host_draw(zero, SEED, row, c, pi, rep) == want
            assert ref.host_draw(None, SEED, row, c, pi, rep) == want
    # the rule's corner: an entry below epsneg is never drawn, the last category takes the remainder
    p = np.array([1e-12, 1e-12, 1.0], np.float32)
    assert all(ref.host_draw(zero, SEED, 0, c, p, p) == (2, 2) for c in range(64))
