"""Numpy restatement of the device exploration policy's draw rule (include/manette_hip.h, mt_policy),
shared by tests/test_policy_cpu.py and tests/test_policy_gpu.py: mix64 on np.uint64, the epsilon rule
in Python floats, the three choosers; and a ctypes wrapper of the host restatement mt_policy_draw_host."""
import ctypes as C
import math

import numpy as np

EPSNEG = np.float32(np.finfo(np.float32).epsneg)
MULTINOMIAL, EGREEDY, ARGMAX = 0, 1, 2
_U = np.uint64


def mix64(z):
    z = np.asarray(z, dtype=_U)
    with np.errstate(over='ignore'):
        z = (z ^ (z >> _U(30))) * _U(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> _U(27))) * _U(0x94d049bb133111eb)
        return z ^ (z >> _U(31))


def uniforms(seed, row, counter):
    """(ua, ur) of (seed, global row, counter); row / counter scalars or arrays."""
    row, counter = np.asarray(row, dtype=_U), np.asarray(counter, dtype=_U)
    with np.errstate(over='ignore'):
        h = mix64(_U(seed) ^ mix64((row << _U(40)) ^ counter))
        h2 = mix64(h ^ _U(0x9e3779b97f4a7c15))
    scale = 2.0 ** -53
    return (h >> _U(11)).astype(np.float64) * scale, (h2 >> _U(11)).astype(np.float64) * scale


def policy(mode=MULTINOMIAL, epsilon=0.0, annealed=False, annealing_steps=0.0, rows_per_call=None):
    from manette_amd import _lib
    if rows_per_call is None:  # (policy() is the zero-filled struct)
        rows_per_call = 0 if mode == MULTINOMIAL else 1
    return _lib.mt_policy(mode, int(annealed), epsilon, annealing_steps, rows_per_call)


def epsilon_of(pol, counter):
    """The epsilon of the call that reads `counter` (exploration_policy.py:73-76), Python floats."""
    if pol.mode != EGREEDY:
        return 0.0
    if not pol.annealed:
        return float(pol.epsilon)
    g = float((int(counter) * int(pol.rows_per_call)) & (2 ** 64 - 1))  # (a uint64 product)
    if g <= pol.annealing_steps:
        return pol.epsilon - (g * pol.epsilon / pol.annealing_steps)
    return 0.0


def multinomial_index(p, u):
    p = np.asarray(p, np.float32)
    cum = 0.0
    for j in range(len(p) - 1):
        cum += float(np.float32(p[j] - EPSNEG))
        if u < cum:
            return j
    return len(p) - 1


def choose_index(p, u, eps):
    n = len(p)
    if u < eps:
        return min(n - 1, int(math.floor((u / eps) * n)))
    return int(np.argmax(np.asarray(p, np.float32)))  # first maximum; the first NaN wins


def draw(pol, seed, row, counter, pi, rep):
    """(a, r) of one row by the rule; pol None = multinomial."""
    ua, ur = (float(x) for x in uniforms(seed, row, counter))
    if pol is None or pol.mode == MULTINOMIAL:
        return multinomial_index(pi, ua), multinomial_index(rep, ur)
    eps = epsilon_of(pol, counter)
    return choose_index(pi, ua, eps), choose_index(rep, ur, eps)


def host_draw(pol, seed, row, counter, pi, rep, expect=0):
    """mt_policy_draw_host; returns (a, r), or the status when expect != 0."""
    from manette_amd import _lib
    pi = np.ascontiguousarray(pi, np.float32)
    rep = np.ascontiguousarray(rep, np.float32)
    a, r = C.c_int32(-1), C.c_int32(-1)
    rc = _lib.hip().mt_policy_draw_host(None if pol is None else C.byref(pol), seed, row, counter,
                                        pi.ctypes.data_as(C.c_void_p), len(pi), rep.ctypes.data_as(C.c_void_p),
                                        len(rep), C.byref(a), C.byref(r))
    if expect:
        return rc
    assert rc == 0, _lib.hip().mt_last_error()
    return a.value, r.value


def special_rows(n):
    """(name, row, first-maximum index): the tie / last / NaN / all-equal rows of size n (n >= 3)."""
    base = np.linspace(0.01, 0.02, n).astype(np.float32)
    tie = base.copy()
    tie[1] = tie[n - 1] = 0.5
    last = base.copy()
    last[n - 1] = 0.9
    nan = base.copy()
    nan[0] = 0.9
    nan[1] = nan[n - 1] = np.nan
    return [('tie', tie, 1), ('last', last, n - 1), ('nan', nan, 1), ('equal', np.full(n, 1.0 / n, np.float32), 0)]
