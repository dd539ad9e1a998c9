"""PAACLearner on the BAYESIAN arch (E = 8, T = 5, synthetic emulators): the Python step with host or
device sampling, the update with the train step's fresh mask, determinism, one update against the
oracles (the checks of tests/test_e2e_gpu.py), and the CLIs."""
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


def _learner(tmp, sampling, staging, seed=0, ec=8):
    sys.path.insert(0, ROOT)
    import train as cli
    from manette_amd.exploration_policy import ExplorationPolicy
    from manette_amd.paac import PAACLearner
    a = cli.get_arg_parser().parse_args([])
    a.game, a.arch, a.emulator_counts, a.emulator_workers = 'pong', 'BAYESIAN', ec, 2
    a.keep_percentage = KEEP
    a.runner, a.sampling, a.seed, a.staging, a.pipeline = 'native', sampling, seed, staging, True
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


def _run(L, updates):
    for _ in range(updates):
        L.book.new_update()
        L.rollout()
        L.update()
    torch.cuda.synchronize()


def _state(L):
    c = lambda t: t.cpu().numpy().copy()
    return dict(params=c(L.network.params), ms=c(L.network.ms), states=c(L.states), gs=L.global_step)


@pytest.mark.parametrize('sampling,staging', [('host', 'in_place'), ('device', 'resized')])
def test_four_updates_run_and_repeat(tmp_path, sampling, staging):
    out = []
    for name, seed in (('a', 0), ('b', 0), ('c', 1)):
        L = _learner(tmp_path / name, sampling, staging, seed=seed)
        try:
            # never the native macro-step, a captured update or the staging that assumes them
            assert L.native_step is None and not L._graph_ok() and not L.boot_in_rollout
            assert staging == 'in_place' or not L.runners.fixed_slots
            _run(L, 4)
            assert L._graphs is None and L.global_step == 4 * 5 * 8
            out.append(_state(L))
        finally:
            L.cleanup()
    a, b, c = out
    for k in ('params', 'ms', 'states'):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert np.isfinite(a['params']).all() and (a['params'] != c['params']).any()


def test_update_matches_oracles(tmp_path):
    L = _learner(tmp_path, 'device', 'resized')
    try:
        net = L.network
        E, T, A, R = L.emulator_counts, L.max_local_steps, L.num_actions, L.total_repetitions
        N = E * T
        _run(L, 3)
        c = lambda t: t.detach().cpu().numpy().copy()
        P = net.get_variables()
        flat_p, ms0, mom0 = c(net.params), c(net.ms), c(net.mom)
        L.book.new_update()
        L.rollout()
        torch.cuda.synchronize()
        states, rm, values, idx = c(L.states), L.rm_h.numpy().copy(), c(L.values), L.idx_h.numpy().copy()
        roll_mask = net.dropout_mask(L.train_ws, N)
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
    finally:
        L.cleanup()
    # the train step drew a fresh mask over the rollout's rows
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


def test_train_and_eval_clis(tmp_path):
    df = str(tmp_path / 'run') + '/'
    cmd = [sys.executable, os.path.join(ROOT, 'train.py'), '-g', 'pong', '--arch', 'BAYESIAN', '--keep_percentage',
           str(KEEP), '-ec', '8', '-ew', '2', '--sampling', 'device', '--max_global_steps', '240',
           '--checkpoint_interval', '120', '-df', df]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    from manette_amd import tf_bundle
    z = tf_bundle.read_bundle(df + 'checkpoints/-240')
    assert z['Network_1/fc4/fc4_weights'].shape == (256, 256) and 'Network_1/fc4/fc4_biases/OptimizerVariables' in z
    ev = subprocess.run([sys.executable, os.path.join(ROOT, 'test.py'), '-f', df, '-tc', '2', '-np', '3'],
                        capture_output=True, text=True, timeout=300)
    assert ev.returncode == 0, ev.stdout[-2000:] + ev.stderr[-2000:]
    assert 'Restoring network variables' in ev.stdout + ev.stderr
    lines = ev.stdout.splitlines()
    assert 'Performed 2 tests for pong.' in lines and any(l.startswith('Mean: ') for l in lines)
