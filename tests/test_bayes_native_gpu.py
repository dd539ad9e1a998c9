"""--bayes_native: the BAYESIAN learner on the native pipelined macro-step (MT_ROLLOUT_DROPOUT) with the
update captured around mt_dropout_returns_loss_backward (synthetic emulators, ew = 2): native ==
Python step, fresh masks from the replayed rollout graph, one replayed update against the oracles,
the device exploration policy, the CLIs, and the data-parallel form of the update at world 1."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bayes_ref
import parity_util
from oracle import optim, returns

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEEP = 0.8
TRAIN_SALT = 0x7452414e5f575321  # paac.py: the train workspace's stream is the sample seed under this salt


def _learner(tmp, staging='resized', pipeline=True, ec=8, t_max=5, native=True, seed=0, egreedy=False, dp_force=False):
    sys.path.insert(0, ROOT)
    import train as cli
    from manette_amd.exploration_policy import ExplorationPolicy
    from manette_amd.paac import PAACLearner
    a = cli.get_arg_parser().parse_args(['--arch', 'BAYESIAN'] + (['--bayes_native'] if native else []))
    a.game, a.emulator_counts, a.emulator_workers, a.max_local_steps = 'pong', ec, 2, t_max
    a.keep_percentage = KEEP
    a.runner, a.sampling, a.seed, a.staging, a.pipeline = 'native', 'device', seed, staging, pipeline
    if egreedy:
        a.egreedy, a.epsilon, a.annealed, a.annealed_steps = True, 0.3, True, 96
    a.dp_force = dp_force
    a.debugging_folder = str(tmp) + '/'
    a.max_global_steps = 1 << 40
    a.checkpoint_interval = 1 << 40
    a.lr_annealing_steps = 100000
    np.random.seed(1234)
    explo = ExplorationPolicy(a)
    nc, ec_ = cli.get_network_and_environment_creator(a, explo)
    L = PAACLearner(nc, ec_, explo, a)
    L.start()
    return L


def _python_step(L):
    from manette_amd import _lib
    _lib.hip().mt_rollout_destroy(L.native_step)
    L.native_step = None
    return L


def _run(L, updates, rec=None):
    for _ in range(updates):
        L.book.new_update()
        L.rollout()
        L.update()
        if rec is not None:
            torch.cuda.synchronize()
            rec.append(L.idx_h.numpy().copy())
    torch.cuda.synchronize()


def _state(L):
    # (slot 0 is excluded: the native stacking step carries slot T over inside the next step 0's forward)
    c = lambda t: t.cpu().numpy().copy()
    return dict(params=c(L.network.params), ms=c(L.network.ms), states=c(L.states[1:]), gs=L.global_step)


def _update_form(L):
    from manette_amd import _lib
    form = C.c_int(-1)
    _lib.check(_lib.hip().mt_rollout_update_form(L.native_step, C.byref(form)), 'mt_rollout_update_form')
    return form.value


def _host_masks(seed, row0, rows, counter):
    from manette_amd import _lib
    out = np.zeros((rows, 256), np.uint8)
    for b in range(rows):
        _lib.check(_lib.hip().mt_dropout_mask_host(seed, row0 + b, counter, KEEP, out[b].ctypes.data_as(C.c_void_p)))
    return out


def _python_reference(tmp, ec, t_max, updates, **kw):
    B = _python_step(_learner(tmp, staging='copy', pipeline=False, ec=ec, t_max=t_max, **kw))
    try:
        assert B.bayes_native and not B._graph_ok()
        rec = []
        _run(B, updates, rec)
        assert B._graphs is None
        return _state(B), rec
    finally:
        B.cleanup()


_REF = {}


def _reference(tmp_path_factory, ec, t_max):
    """The Python step's 6 updates at (ec, t_max), computed once and shared (never modified)."""
    k = (ec, t_max)
    if k not in _REF:
        _REF[k] = _python_reference(tmp_path_factory.mktemp('ref_%d_%d' % k), ec, t_max, 6)[0]
    return _REF[k]


@pytest.mark.parametrize('staging,pipeline,ec,t_max', [('resized', True, 8, 5), ('zero_copy', True, 8, 5),
                                                       ('in_place', False, 8, 5), ('resized', True, 5, 2),
                                                       ('resized', True, 17, 1)])
def test_native_step_equals_python_step(tmp_path, tmp_path_factory, staging, pipeline, ec, t_max):
    """A = the flag with the native macro-step, B = the flag with staging copy and the Python step: after
    6 updates the states, parameters and RMSProp slots differ in zero elements. (5, 2) and (17, 1): a
    ragged pull block and ragged 16-row stage tiles."""
    A = _learner(tmp_path / 'a', staging=staging, pipeline=pipeline, ec=ec, t_max=t_max)
    try:
        assert A.bayes_native and A.native_step is not None
        assert A.boot_in_rollout == pipeline and A._boot_ws is None
        assert staging == 'in_place' or A.runners.fixed_slots
        if staging == 'resized':
            assert A.slot0_in_rollout and A._graph_ok()
        _run(A, 6)
        if staging == 'resized':  # the path: one captured update, launched by the rollout's last step
            assert A._graphs is not None and len(A._graphs) == 1 and A._buckets is None
            assert A._update_in_rollout and A._rollout_update == 'all' and _update_form(A) == 1
        elif pipeline:
            assert A._graphs is not None and A._update_in_rollout
        else:
            assert A._graphs is None and not A._update_in_rollout
        sa = _state(A)
    finally:
        A.cleanup()
    sb = _reference(tmp_path_factory, ec, t_max)
    bad = {k: int(np.sum(sa[k] != sb[k])) for k in ('states', 'params', 'ms')}
    assert not any(bad.values()), bad
    assert sa['gs'] == sb['gs'] == 6 * t_max * ec
    assert np.isfinite(sa['params']).all()


def test_replayed_rollout_graph_draws_fresh_masks(tmp_path):
    """E = 5, T = 2, keep 0.8: the third rollout runs from the replayed rollout graph (captured by the
    second); its train rows hold the masks of the rollout workspace's stream at counters 2 (T + 1) + t —
    every forward and the bootstrap consumed one counter value per row, none of it a kernel argument."""
    E, T = 5, 2
    L = _learner(tmp_path, ec=E, t_max=T)
    try:
        L.use_update_graph = False  # (eager updates, launched after the masks are read)
        masks = []
        for n in range(3):
            L.book.new_update()
            L.rollout()
            torch.cuda.synchronize()
            masks.append(L.network.dropout_mask(L.train_ws, T * E))
            seed, row0, cnt = L.network.dropout_state(L.network.workspace(E, 'rollout'), E)
            assert (seed, row0) == (L.sample_seed, L.env_offset) and (cnt == (n + 1) * (T + 1)).all()
            L.update()
        torch.cuda.synchronize()
        seed, off = L.sample_seed, L.env_offset
    finally:
        L.cleanup()
    for n in range(3):
        for t in range(T):
            np.testing.assert_array_equal(masks[n][t * E:(t + 1) * E], _host_masks(seed, off, E, n * (T + 1) + t),
                                          err_msg='rollout %d step %d' % (n, t))
    assert (masks[2] != masks[1]).any()


def test_replayed_update_matches_oracles(tmp_path):
    """The checks of test_bayes_learner_gpu.test_update_matches_oracles on the native path: E = 8, T = 5,
    the fourth update — a graph replay launched by the rollout's last step."""
    L = _learner(tmp_path)
    try:
        net = L.network
        E, T, A, R = L.emulator_counts, L.max_local_steps, L.num_actions, L.total_repetitions
        N = E * T
        _run(L, 3)
        assert L._graphs is not None and L._update_in_rollout
        c = lambda t: t.detach().cpu().numpy().copy()
        P = net.get_variables()
        flat_p, ms0, mom0 = c(net.params), c(net.ms), c(net.mom)
        L.book.new_update()
        L.rollout()  # (its last step launched the update)
        torch.cuda.synchronize()
        states, rm, values, idx = c(L.states), L.rm_h.numpy().copy(), c(L.values), L.idx_h.numpy().copy()
        gs = L.global_step
        L.update()
        torch.cuda.synchronize()
        dev = net.forward_branches(L.train_ws, 0, N)
        v_boot, v_upd, pi_upd, rep_upd = c(L.v_boot), c(L.v_upd), c(L.pi_upd), c(L.rep_upd)
        grad, y, adv, grad_flat = net.get_variables('grad'), c(L.y), c(L.adv), c(net.grad)
        w1, ms1, mom1 = c(net.params), c(net.ms), c(net.mom)
        norm_dev, lr_dev, terms = float(net.norm_dev.item()), float(net._lr_host[0]), c(L.loss_terms)
        gamma, beta, clip, decay, eps = L.gamma, net.beta, net.clip_norm, net.decay, net.eps
        lr0 = optim.get_lr(gs, L.initial_lr, L.lr_annealing_steps)
        seed, off = L.sample_seed, L.env_offset
    finally:
        L.cleanup()
    # the train step's mask: the train workspace's stream at its fourth draw, not the rollout's masks
    np.testing.assert_array_equal(dev['mask'], _host_masks(seed ^ TRAIN_SALT, T * off, N, 3))
    roll_mask = np.concatenate([_host_masks(seed, off, E, 3 * (T + 1) + t) for t in range(T)])
    assert (dev['mask'] != roll_mask).any() and (v_upd != values.reshape(N)).any()
    # n-step returns from the ROLLOUT's values (bit-exact)
    y0, adv0 = returns.nstep_returns(rm[0].astype(np.float64), rm[1].astype(np.float64), values.astype(np.float64),
                                     v_boot, gamma)
    np.testing.assert_array_equal(y, y0.astype(np.float32))
    np.testing.assert_array_equal(adv, adv0.astype(np.float32))
    # the train step's outputs and the gradient under ITS mask
    obs = states[:T].reshape(N, 84, 84, -1)
    ref = bayes_ref.forward(P, obs, dev['mask'], KEEP, 1, A, R)
    np.testing.assert_allclose(v_upd, ref[0], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(pi_upd, ref[1], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(rep_upd, ref[2], rtol=2e-5, atol=1e-6)
    br = bayes_ref.branches_checked(ref[3], dev)
    _, G, aux = bayes_ref.loss_and_grads(P, ref[3], ref[0], ref[1], ref[2], idx[0].reshape(N), idx[1].reshape(N),
                                         y.reshape(N), adv.reshape(N), beta, br=br)
    parity_util.check_grads(bayes_ref.spec(1, A, R), grad, G, set())
    np.testing.assert_allclose(terms, aux['terms'], rtol=1e-4, atol=1e-5)
    # global-norm clip + TF1 RMSProp on the device gradient (bit-exact)
    assert np.float32(lr_dev) == np.float32(lr0)
    ref_norm = optim.global_norm([grad_flat])
    assert abs(norm_dev - ref_norm) <= 1e-5 * ref_norm, (norm_dev, ref_norm)
    s = optim.clip_scale(norm_dev, clip)
    w, ms, mom = flat_p.copy(), ms0.copy(), mom0.copy()
    optim.rmsprop_apply(w, ms, mom, grad_flat * s, np.float32(lr_dev), decay, 0.0, eps)
    np.testing.assert_array_equal(ms1, ms)
    np.testing.assert_array_equal(mom1, mom)
    np.testing.assert_array_equal(w1, w)


def test_egreedy_annealed_equals_python_step(tmp_path):
    """--egreedy --annealed with the flag: the fused draw of the native macro-step selects the indices
    the Python step's mt_sample_policy selects, over 4 updates (epsilon reaches 0 at call 12)."""
    A = _learner(tmp_path / 'a', egreedy=True)
    try:
        assert A.native_step is not None and A.policy is not None
        ra = []
        _run(A, 4, ra)
        sa = _state(A)
    finally:
        A.cleanup()
    sb, rb = _python_reference(tmp_path / 'b', 8, 5, 4, egreedy=True)
    for n, (x, y) in enumerate(zip(ra, rb)):
        np.testing.assert_array_equal(x, y, err_msg='indices of rollout %d' % n)
    for k in ('params', 'ms', 'states'):
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    assert len({int(v) for r in ra for v in r[0].reshape(-1)}) > 1


def test_data_parallel_form_at_world_one(tmp_path):
    """The world > 1 form of the update, forced at world 1 (the RCCL sum is the identity): two graphs,
    backward and apply, around one eager whole-gradient all-reduce launched by the learner — never
    bucketed, never launched by the rollout — equal to the Python step under the same form."""
    A = _learner(tmp_path / 'a', dp_force=True)
    try:
        assert A.dp and A.world == 1 and A.native_step is not None
        _run(A, 4)
        assert A._graphs is not None and len(A._graphs) == 2 and A._buckets is None
        assert not A._update_in_rollout and _update_form(A) == 0
        sa = _state(A)
    finally:
        A.cleanup()
    sb, _ = _python_reference(tmp_path / 'b', 8, 5, 4, dp_force=True)
    for k in ('params', 'ms', 'states'):
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)


def test_train_and_eval_clis(tmp_path):
    df = str(tmp_path / 'run') + '/'
    cmd = [sys.executable, os.path.join(ROOT, 'train.py'), '-g', 'pong', '--arch', 'BAYESIAN', '--bayes_native',
           '--keep_percentage', str(KEEP), '-ec', '8', '-ew', '2', '--sampling', 'device', '--max_global_steps', '240',
           '--checkpoint_interval', '120', '-df', df]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'no native macro-step' not in out.stdout + out.stderr
    from manette_amd import tf_bundle
    z = tf_bundle.read_bundle(df + 'checkpoints/-240')
    assert z['Network_1/fc4/fc4_weights'].shape == (256, 256) and 'Network_1/fc4/fc4_biases/OptimizerVariables' in z
    import json
    with open(df + 'args.json') as f:
        assert json.load(f)['bayes_native'] is True
    ev = subprocess.run([sys.executable, os.path.join(ROOT, 'test.py'), '-f', df, '-tc', '2', '-np', '3'],
                        capture_output=True, text=True, timeout=300)
    assert ev.returncode == 0, ev.stdout[-2000:] + ev.stderr[-2000:]
    assert 'Restoring network variables' in ev.stdout + ev.stderr
    lines = ev.stdout.splitlines()
    assert 'Performed 2 tests for pong.' in lines and any(l.startswith('Mean: ') for l in lines)

    # the flag with another arch: refused before anything is allocated
    bad = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--arch', 'NIPS', '--bayes_native', '-df',
                          str(tmp_path / 'bad') + '/'], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and 'bayes_native' in bad.stderr
