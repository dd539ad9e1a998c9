"""Kernel parity along the axes the other GPU modules hold fixed: softmax temperature, leaky ReLU
off the NIPS path, the loss / return / optimizer scalars, the head and scan sizes at the limits
mt_net_create and mt_returns_loss_backward accept, and the exports without a test of their own
(mt_preprocess_frames, mt_sum_slabs).

Bounds are the project's: forward 2e-5, gradients 2e-4 relative L2 per variable and per channel
(parity_util.check_grads), per-row loss terms 1e-4; integer work and everything the oracle restates
operation by operation (returns, RMSProp, slab sums) bit for bit. Shapes are the smallest that
reach the path. tests/test_oracle_torch.py pins the oracle's temperature / alpha handling against
torch autograd first.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nets, optim, preprocess, returns

pytestmark = pytest.mark.gpu

ACTOR_W = 'Training/Actor/actor_output/actor_output_weights'
REP_W = 'Training/Repetition/repetition_output/repetition_output_weights'

# After the default init (U(+-1/sqrt(F)) head weights) the logits are nearly flat: softmax(z / temp)
# is then ~uniform at every temp, and a kernel that ignored the temperature, or an entropy term of
# the wrong weight, would hide inside the bounds. The softmax heads' weights are therefore scaled by
# a constant, chosen on the CPU from the oracle alone (nets.forward at temp = 0.5 on the cases of
# test_softmax_temperature) so that some row's largest pi exceeds 0.5 while every probability stays
# above 1e-6 (clear of fp32 exp underflow, which the loss's 1e-30 epsilon would turn into a different
# test). One constant cannot do both for every arch: the LSTM's dense layer reads the N(0, 1)
# projection (features of order 1; at 8 its smallest probability is 3e-10), the conv archs' heads
# need 70 or more (NIPS 6 x 1 at 64: max pi 0.48; NIPS 9 x 11 at 128: smallest probability 6e-8).
# 80 -> (max pi, smallest probability) = (0.56, 1.4e-2) NIPS 6 x 1, (0.89, 2.7e-5) NIPS 9 x 11,
# (0.62, 2.0e-2) NATURE 4 x 11;  2 -> (0.83, 1.1e-3) LSTM 9 x 11.
# The float32 oracle's own error against its float64 self on these cases: gradients <= 3.2e-6 relative
# L2 (per channel 1.2e-6), pi / rep 3.5e-6 relative, loss terms 1e-6 — 4 x that is inside the project's
# bounds, so no case's bound is widened.
HEAD_SCALE = {'NIPS': 80.0, 'NATURE': 80.0, 'LSTM': 2.0}


def _make(arch, depth, A, R, seed, **kw):
    """A DeviceNetwork through the other modules' helpers (LSTM: tests/test_lstm_gpu.py's, with its
    non-zero cell bias)."""
    if arch == 'LSTM':
        from test_lstm_gpu import _net
        return _net(depth, A, R, seed, **kw)
    from test_kernels_gpu import _net
    return _net(arch, depth, A, R, seed=seed, **kw)


def _scale_heads(net):
    P = net.get_variables()
    c = np.float32(HEAD_SCALE[net.arch])
    net.set_variables({k: (P[k] * c).astype(np.float32) for k in (ACTOR_W, REP_W)})


def _obs(rs, arch, depth, B):
    if arch == 'LSTM':
        from test_lstm_gpu import _windows
        return _windows(rs, B, depth)
    return rs.randint(0, 256, size=(B, 84, 84, 4 * depth)).astype(np.uint8)


def _targets(rs, A, R, B):
    return (rs.randint(0, A, size=B).astype(np.int32), rs.randint(0, R, size=B).astype(np.int32),
            rs.randn(B).astype(np.float32), rs.randn(B).astype(np.float32))


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _check_forward(got, ref):
    (v, pi, rep), (v0, pi0, rep0) = got, ref
    np.testing.assert_allclose(v.cpu().numpy().reshape(-1), v0, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(pi.cpu().numpy().reshape(pi0.shape), pi0, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(rep.cpu().numpy().reshape(rep0.shape), rep0, rtol=2e-5, atol=1e-6)


def _padding_is_zero(net):
    flat = net.grad.cpu().numpy()
    mask = np.ones(net.nparams, bool)
    for _, shape, off, _ in net.vars:
        mask[off:off + int(np.prod(shape))] = False
    assert not flat[mask].any()


def _parity(net, arch, depth, A, R, obs, tgt, act='relu', alpha=0.1, temp=1.0, beta=0.02, infer=True):
    """forward, forward(infer=True) and loss_backward (+ per-row loss terms) of `net` on obs against
    the oracle at the project's bounds; the oracle follows the device's branches at the gradient's
    discontinuities (parity_util.device_branches checks them away from near-ties). Returns the
    oracle's (v, pi, rep)."""
    import parity_util
    a_idx, r_idx, y, adv = tgt
    B = len(obs)
    obs_d = _d(obs)
    spec = nets.arch_spec(arch, depth, A, R)
    P = net.get_variables()
    ref = nets.forward(spec, P, obs, act=act, alpha=alpha, temp=temp)[:3]
    if infer:
        _check_forward([t.clone() for t in net.forward(obs_d, infer=True, ws_key=('axes_infer', B))], ref)
    v, pi, rep = net.forward(obs_d)
    terms = torch.zeros(B, 4, device='cuda')
    net.loss_backward(obs_d, B, v, pi, rep, _d(a_idx), _d(r_idx), _d(y), _d(adv), loss_terms=terms)
    torch.cuda.synchronize()
    _check_forward((v, pi, rep), ref)
    if arch == 'LSTM':
        frames = obs.reshape((-1,) + obs.shape[2:])
        dev = net.forward_branches(net.workspace(B), 2, B)
    else:
        frames, dev = obs, net.forward_branches(net.workspace(B), 0, B)
    br = parity_util.device_branches(spec, P, frames, dev, act, alpha)
    _, G, aux = nets.loss_and_grads(spec, P, obs, a_idx, r_idx, y, adv, beta, act=act, alpha=alpha, temp=temp,
                                    routes=br['routes'], branches=br['branches'], hbranch=br['hbranch'])
    parity_util.check_grads(spec, net.get_variables('grad'), G, set())
    np.testing.assert_allclose(terms.cpu().numpy(), aux['terms'], rtol=1e-4, atol=1e-5)
    _padding_is_zero(net)
    return ref


# ---------------------------------------------------------------------------------------------------
# 2. softmax temperature
# ---------------------------------------------------------------------------------------------------
TEMP_CONFIGS = [('NIPS', 1, 6, 1), ('NIPS', 1, 9, 11), ('NATURE', 1, 4, 11), ('LSTM', 1, 9, 11)]


def _temp_case(arch, depth, A, R):
    """Seed, observations and targets of a temperature case (shared with the CPU calibration of
    HEAD_SCALE: nets.init_params draws the stream DeviceNetwork.init_params draws)."""
    seed = 50 + A + R
    rs = np.random.RandomState(seed)
    B = 5
    return seed, _obs(rs, arch, depth, B), _targets(rs, A, R, B)


@pytest.mark.parametrize('temp', [0.5, 2.0])
@pytest.mark.parametrize('arch,depth,A,R', TEMP_CONFIGS)
def test_softmax_temperature(arch, depth, A, R, temp):
    """heads_row's `temp != 1` branch, head_softmax_grad's `/ temp` and the LSTM heads at
    softmax_temp 0.5 and 2.0 with the softmax heads scaled by HEAD_SCALE, so the policy at temp is
    far from the policy at 1: forward, infer forward, gradients and per-row loss terms vs the
    oracle. ('NIPS', 1, 6, 1): the R == 1 shortcut beside a real temperature.)"""
    seed, obs, tgt = _temp_case(arch, depth, A, R)
    net = _make(arch, depth, A, R, seed, temp=temp)
    _scale_heads(net)
    spec = nets.arch_spec(arch, depth, A, R)
    P = net.get_variables()
    # the calibration conditions of HEAD_SCALE, on the oracle's output at temp = 0.5
    _, pi5, rep5, _ = nets.forward(spec, P, obs, temp=0.5)
    assert pi5.max(axis=1).max() > 0.5, pi5.max(axis=1)
    assert min(pi5.min(), rep5.min()) > 1e-6, (pi5.min(), rep5.min())
    ref = _parity(net, arch, depth, A, R, obs, tgt, temp=temp)
    # and the temperature shows: the same parameters at temp = 1 are another policy, well outside 2e-5
    _, pi1, _, _ = nets.forward(spec, P, obs, temp=1.0)
    assert np.abs(ref[1] - pi1).max() > 1e-2


# ---------------------------------------------------------------------------------------------------
# 3. leaky ReLU off the NIPS path
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', [0.1, 0.3])
@pytest.mark.parametrize('arch,depth,A,R', [('NATURE', 1, 4, 11), ('PWYX', 1, 4, 11), ('PWYX', 3, 6, 1)])
def test_leaky_relu_rows_then_backward(arch, depth, A, R, alpha):
    """activation = leaky_relu on NATURE's direct convs (dconv.h act_fwd / act_bwd, nature_bwd.h)
    and PWYX's pooled layers (activation, max-pool argmax, DBwdUnpool): mt_forward_rows of 3 + 2
    rows into one 5-row train workspace, mt_forward and mt_forward_infer on the same rows, then
    mt_loss_backward on the train workspace with no forward — outputs and gradients vs the oracle,
    which follows the device's `>= 0` branches and pooled argmax (device_branches(act, alpha))."""
    import parity_util
    act, B = 'leaky_relu', 5
    net = _make(arch, depth, A, R, 60 + A + depth, act=act, alpha=alpha)
    rs = np.random.RandomState(61 + depth + int(alpha * 10))
    obs = _obs(rs, arch, depth, B)
    a_idx, r_idx, y, adv = _targets(rs, A, R, B)
    obs_d = _d(obs)
    spec = nets.arch_spec(arch, depth, A, R)
    P = net.get_variables()
    ref = nets.forward(spec, P, obs, act=act, alpha=alpha)[:3]
    _check_forward([t.clone() for t in net.forward(obs_d, infer=True, ws_key='leaky_infer')], ref)
    _check_forward([t.clone() for t in net.forward(obs_d, ws_key='leaky_plain')], ref)
    tws = net.workspace(B, 'leaky_train')
    v = torch.zeros(B, device='cuda')
    pi = torch.zeros(B, A, device='cuda')
    rep = torch.zeros(B, R, device='cuda')
    for r0, n in ((0, 3), (3, 2)):
        net.forward_rows(obs_d[r0:r0 + n], n, tws, B, r0, out=(v[r0:r0 + n], pi[r0:r0 + n], rep[r0:r0 + n]),
                         ws_key=('leaky_rows', n))
    terms = torch.zeros(B, 4, device='cuda')
    net.loss_backward(obs_d, B, v, pi, rep, _d(a_idx), _d(r_idx), _d(y), _d(adv), loss_terms=terms,
                      ws_key='leaky_train')
    torch.cuda.synchronize()
    _check_forward((v, pi, rep), ref)
    br = parity_util.device_branches(spec, P, obs, net.forward_branches(tws, 0, B), act, alpha)
    _, G, aux = nets.loss_and_grads(spec, P, obs, a_idx, r_idx, y, adv, 0.02, act=act, alpha=alpha,
                                    routes=br['routes'], branches=br['branches'], hbranch=br['hbranch'])
    parity_util.check_grads(spec, net.get_variables('grad'), G, set())
    np.testing.assert_allclose(terms.cpu().numpy(), aux['terms'], rtol=1e-4, atol=1e-5)


def _pinned_rewards(rs, T, E, zero_frac):
    """[2][T][E] pinned: rewards in {-1, 0, 1}, masks with ~zero_frac zeros; and its device address."""
    from manette_amd.network import host_device_pointer
    rm = torch.zeros(2, T, E, dtype=torch.float32).pin_memory()
    rm[0] = torch.from_numpy(rs.choice([-1.0, 0.0, 1.0], size=(T, E)).astype(np.float32))
    rm[1] = torch.from_numpy((rs.rand(T, E) > zero_frac).astype(np.float32))
    return rm, host_device_pointer(rm)


def _fused(net, obs, T, E, pi, rep, v, a_idx, r_idx, rm_dev, v_boot, gamma, boot_ws=None):
    """mt_returns_loss_backward[_boot] from a zeroed gradient: (y, adv, loss terms, grad)."""
    N = T * E
    y, adv = torch.empty(T, E, device='cuda'), torch.empty(T, E, device='cuda')
    lt = torch.empty(N, 4, device='cuda')
    net.grad.zero_()
    net.returns_loss_backward(obs, T, E, pi, rep, v, a_idx, r_idx, rm_dev, rm_dev + 4 * N, v_boot, gamma, y, adv,
                              loss_terms=lt, boot_ws=boot_ws)
    torch.cuda.synchronize()
    return y.clone(), adv.clone(), lt.clone(), net.grad.clone()


def _unfused(net, obs, T, E, pi, rep, v, a_idx, r_idx, rm_dev, v_boot, gamma):
    """mt_returns, then mt_loss_backward, from a zeroed gradient: (y, adv, loss terms, grad)."""
    from manette_amd.network import returns as dev_returns
    N = T * E
    y, adv = torch.empty(T, E, device='cuda'), torch.empty(T, E, device='cuda')
    lt = torch.empty(N, 4, device='cuda')
    net.grad.zero_()
    dev_returns(rm_dev, rm_dev + 4 * N, v.view(T, E), v_boot, gamma, y, adv)
    net.loss_backward(obs, N, v, pi, rep, a_idx, r_idx, y.view(N), adv.view(N), loss_terms=lt)
    torch.cuda.synchronize()
    return y.clone(), adv.clone(), lt.clone(), net.grad.clone()


def _same(a, b):
    for x, z, k in zip(a, b, ('y', 'adv', 'loss_terms', 'grad')):
        np.testing.assert_array_equal(x.cpu().numpy(), z.cpu().numpy(), err_msg=k)


@pytest.mark.parametrize('act', ['relu', 'leaky_relu'])
@pytest.mark.parametrize('arch,A,R', [('NIPS', 6, 1), ('NATURE', 4, 11)])
def test_boot_value_in_loss_kernel(arch, A, R, act):
    """mt_returns_loss_backward_boot without the rollout: the E-row workspace mt_forward_trunk leaves
    holds the dense layer's split-K slabs where MT_ROLLOUT_BOOT_SLABS leaves them (ws_layout(E).fcslab,
    the same slab count: both go through the arch's trunk + launch_fc / the fused NIPS trunk), so it
    is a valid boot_ws. boot_value (slab sum, bias, the activation — applied by the loss kernel
    itself — and the critic's dot product) must give V(s_T) of mt_forward_infer's heads, and with it
    y, adv, the loss terms and the gradient of mt_returns_loss_backward given that v_boot: all bit
    for bit; V(s_T) also vs the oracle."""
    T, E = 3, 5
    N = T * E
    net = _make(arch, 1, A, R, 70 + A, act=act)
    rs = np.random.RandomState(71 + A + len(act))
    obs = _obs(rs, arch, 1, N)
    obs_T = _obs(rs, arch, 1, E)
    a_idx, r_idx = _d(rs.randint(0, A, N).astype(np.int32)), _d(rs.randint(0, R, N).astype(np.int32))
    rm, rm_dev = _pinned_rewards(rs, T, E, 0.2)
    rm[1, T - 1, 0] = 1.0  # (the bootstrap reaches at least this return)
    obs_d, obsT_d = _d(obs), _d(obs_T)
    v, pi, rep = [t.clone() for t in net.forward(obs_d)]
    vb = net.forward(obsT_d, infer=True, ws_key='boot_infer')[0].clone()
    net.forward_trunk(obsT_d, E, ws_key='boot_trunk')
    boot_ws = net.workspace(E, 'boot_trunk')
    ref = _fused(net, obs_d, T, E, pi, rep, v, a_idx, r_idx, rm_dev, vb, 0.99)
    vb1 = torch.full((E,), float('nan'), device='cuda')
    got = _fused(net, obs_d, T, E, pi, rep, v, a_idx, r_idx, rm_dev, vb1, 0.99, boot_ws=boot_ws)
    np.testing.assert_array_equal(vb1.cpu().numpy(), vb.cpu().numpy(), err_msg='v_boot')
    _same(ref, got)
    spec = nets.arch_spec(arch, 1, A, R)
    v0 = nets.forward(spec, net.get_variables(), obs_T, act=act, alpha=0.1)[0]
    np.testing.assert_allclose(vb1.cpu().numpy(), v0, rtol=2e-5, atol=2e-5)
    assert ref[0][T - 1, 0].item() != rm[0, T - 1, 0].item()


# ---------------------------------------------------------------------------------------------------
# 4. loss and optimizer scalars
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [0.0, 0.5])
@pytest.mark.parametrize('arch,depth,A,R', [('NIPS', 1, 6, 1), ('NATURE', 1, 4, 11)])
def test_entropy_beta(arch, depth, A, R, beta):
    """entropy_regularisation_strength 0 and 0.5 (everywhere else 0.02): gradients and per-row loss
    terms vs the oracle. The softmax heads are scaled by HEAD_SCALE: at the default init's ~uniform
    policies the entropy's gradient vanishes whatever its weight."""
    import parity_util
    net = _make(arch, depth, A, R, 80 + A, beta=beta)
    _scale_heads(net)
    rs = np.random.RandomState(81 + A)
    B = 5
    obs, tgt = _obs(rs, arch, depth, B), _targets(rs, A, R, B)
    _parity(net, arch, depth, A, R, obs, tgt, beta=beta, infer=False)
    # beta shows: the oracle's actor gradient at the other value is well outside the bound
    spec = nets.arch_spec(arch, depth, A, R)
    P = net.get_variables()
    Ga = nets.loss_and_grads(spec, P, obs, *tgt, beta)[1]
    Gb = nets.loss_and_grads(spec, P, obs, *tgt, 0.5 - beta)[1]
    assert parity_util.rel(Gb[ACTOR_W], Ga[ACTOR_W]) > 1e-2


@pytest.mark.parametrize('gamma', [0.0, 0.5, 1.0])
def test_gamma(gamma):
    """gamma 0, 0.5 and 1 (everywhere else 0.99) at (T, E) = (5, 4): mt_returns vs the oracle's scan
    bit for bit, and mt_returns_loss_backward == mt_returns + mt_loss_backward bit for bit."""
    T, E, A, R = 5, 4, 6, 1
    N = T * E
    net = _make('NIPS', 1, A, R, 90)
    rs = np.random.RandomState(91 + int(gamma * 2))
    obs_d = _d(_obs(rs, 'NIPS', 1, N))
    v, pi, rep = [t.clone() for t in net.forward(obs_d)]
    a_idx, r_idx = _d(rs.randint(0, A, N).astype(np.int32)), _d(rs.randint(0, R, N).astype(np.int32))
    rm, rm_dev = _pinned_rewards(rs, T, E, 0.2)
    VT = rs.randn(E).astype(np.float32)
    ref = _unfused(net, obs_d, T, E, pi, rep, v, a_idx, r_idx, rm_dev, _d(VT), gamma)
    got = _fused(net, obs_d, T, E, pi, rep, v, a_idx, r_idx, rm_dev, _d(VT), gamma)
    _same(ref, got)
    y0, adv0 = returns.nstep_returns(rm[0].numpy().astype(np.float64), rm[1].numpy().astype(np.float64),
                                     v.cpu().numpy().reshape(T, E).astype(np.float64), VT, gamma)
    np.testing.assert_array_equal(ref[0].cpu().numpy(), y0.astype(np.float32))
    np.testing.assert_array_equal(ref[1].cpu().numpy(), adv0.astype(np.float32))


def _clip_rmsprop(g, w, ms, mom, lr, decay, momentum, eps, clip, clip_type, inv_scale):
    """mt_grad_sumsq + mt_clip_rmsprop through the C ABI on copies of the arrays:
    (w, ms, mom, norm) after the update."""
    from manette_amd import _lib
    from manette_amd.network import host_device_pointer
    lib = _lib.hip()
    n = g.size
    gd, wd, msd, momd = _d(g), _d(w), _d(ms), _d(mom)
    partials = torch.zeros(_lib.MT_NORM_PARTIALS, dtype=torch.float32, device='cuda')
    norm = torch.full((1,), float('nan'), device='cuda')
    lr_h = torch.zeros(1, dtype=torch.float32).pin_memory()
    lr_h[0] = float(lr)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.mt_grad_sumsq(p(gd), n, float(inv_scale), p(partials), s), 'mt_grad_sumsq')
    _lib.check(lib.mt_clip_rmsprop(p(wd), p(msd), p(momd), p(gd), n, p(partials), C.c_void_p(host_device_pointer(lr_h)),
                                   float(decay), float(momentum), float(eps), float(clip),
                                   _lib.MT_CLIP[clip_type], float(inv_scale), p(norm), s), 'mt_clip_rmsprop')
    torch.cuda.synchronize()
    return wd.cpu().numpy(), msd.cpu().numpy(), momd.cpu().numpy(), float(norm.item())


def _rmsprop_state(n, seed, gnorm):
    """(g, w, ms, mom): a gradient of global norm gnorm, and non-trivial slots."""
    rs = np.random.RandomState(seed)
    g = rs.randn(n)
    g = (g * (gnorm / np.linalg.norm(g))).astype(np.float32)
    return (g, rs.randn(n).astype(np.float32), (0.5 + rs.rand(n)).astype(np.float32),
            (rs.randn(n) * 1e-3).astype(np.float32))


# (decay, eps, clip, momentum, inv_scale); the gradient's norm is 5 (x 8 before inv_scale = 1/8), so
# clip 0.5 scales it down and clip 40 leaves it alone
RMSPROP_CASES = {
    'decay0.9-eps1e-3': (0.9, 1e-3, 3.0, 0.0, 1.0),
    'clip0.5': (0.99, 0.1, 0.5, 0.0, 1.0),
    'clip40': (0.99, 0.1, 40.0, 0.0, 1.0),
    'momentum0.9': (0.99, 0.1, 3.0, 0.9, 1.0),
    'inv_scale1/8': (0.99, 0.1, 3.0, 0.0, 0.125),
}


@pytest.mark.parametrize('case', sorted(RMSPROP_CASES))
def test_clip_rmsprop_scalars(case):
    """mt_clip_rmsprop away from decay 0.99 / eps 0.1 / clip 3 / momentum 0 / inv_scale 1, called
    through the C ABI (DeviceNetwork passes momentum 0): the norm within 1e-5 relative of the float64
    norm, then ms, mom and params bit for bit against optim.rmsprop_apply given the device's norm.
    n = 100,003: the float4 path's last thread takes the scalar tail. inv_scale = 1/8 (a data-parallel
    sum of 8 ranks): the oracle gets g / 8 (exact), mt_grad_sumsq the same factor."""
    decay, eps, clip, momentum, inv_scale = RMSPROP_CASES[case]
    n, lr = 100003, 0.0224
    g, w, ms, mom = _rmsprop_state(n, 7, 5.0 / inv_scale)
    w1, ms1, mom1, norm = _clip_rmsprop(g, w, ms, mom, lr, decay, momentum, eps, clip, 'global', inv_scale)
    g_eff = g * np.float32(inv_scale)
    ref = optim.global_norm([g_eff])
    assert abs(norm - ref) <= 1e-5 * ref, (norm, ref)
    assert (norm > clip) == (clip < 5.0)  # the clip values straddle the norm
    s = optim.clip_scale(norm, clip)
    assert abs(float(s) - min(1.0, clip / norm)) < 1e-6
    w0, ms0, mom0 = w.copy(), ms.copy(), mom.copy()
    optim.rmsprop_apply(w0, ms0, mom0, g_eff * s, np.float32(lr), decay, momentum, eps)
    np.testing.assert_array_equal(ms1, ms0)
    np.testing.assert_array_equal(mom1, mom0)
    np.testing.assert_array_equal(w1, w0)
    assert not np.array_equal(w1, w)


@pytest.mark.parametrize('momentum', [0.0, 0.9])
def test_clip_rmsprop_zero_gradient(momentum):
    """The all-zero gradient under the global clip: the norm is 0 and 1 / norm is inf, which
    clip * min(1 / norm, 1 / clip) must absorb. No NaN or Inf anywhere; ms decays, and params move by
    the decayed momentum term alone (not at all at momentum 0) — bit for bit the oracle's."""
    n, lr = 100003, 0.0224
    _, w, ms, mom = _rmsprop_state(n, 9, 1.0)
    g = np.zeros(n, np.float32)
    w1, ms1, mom1, norm = _clip_rmsprop(g, w, ms, mom, lr, 0.99, momentum, 0.1, 3.0, 'global', 1.0)
    assert norm == 0.0
    for a in (w1, ms1, mom1):
        assert np.isfinite(a).all()
    s = optim.clip_scale(norm, 3.0)
    assert np.isfinite(s)
    w0, ms0, mom0 = w.copy(), ms.copy(), mom.copy()
    optim.rmsprop_apply(w0, ms0, mom0, g * s, np.float32(lr), 0.99, momentum, 0.1)
    np.testing.assert_array_equal(ms1, ms0)
    np.testing.assert_array_equal(mom1, mom0)
    np.testing.assert_array_equal(w1, w0)
    np.testing.assert_array_equal(w1, w - mom * np.float32(momentum))


# ---------------------------------------------------------------------------------------------------
# 5. limits the library accepts
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', ['fresh', 'after_small_head'])
@pytest.mark.parametrize('arch', ['NIPS', 'NATURE', 'LSTM'])
def test_head_size_limit(arch, order):
    """num_actions = 32, num_reps = 31: 1 + A + R = 64 outputs, a full wave (kMaxHeads), and for
    NATURE (F = 512) a head region of ~129 KB staged in LDS by the heads and loss kernels — past the
    64 KB default, so both raise their dynamic-LDS attribute first (per process, once). Forward at
    B = 3 and forward / infer / loss_backward at B = 5 vs the oracle, in a fresh net and again after
    a small-head net of the same arch has launched both kernels (the order in which an attribute set
    too late, or keyed on the first launch, would show). (With a 150 KB cap the runtime refused the
    loss kernel's attribute — 10.5 KB of static LDS on top is past a CU's 160 KB — and NIPS and
    NATURE raised from mt_loss_backward here.)"""
    A, R = 32, 31
    if order == 'after_small_head':
        small = _make(arch, 1, 4, 3, 100)
        rs = np.random.RandomState(100)
        _parity(small, arch, 1, 4, 3, _obs(rs, arch, 1, 2), _targets(rs, 4, 3, 2))
    net = _make(arch, 1, A, R, 101)
    rs = np.random.RandomState(102)
    obs3 = _obs(rs, arch, 1, 3)
    spec = nets.arch_spec(arch, 1, A, R)
    got = [t.clone() for t in net.forward(_d(obs3))]
    torch.cuda.synchronize()
    _check_forward(got, nets.forward(spec, net.get_variables(), obs3)[:3])
    _parity(net, arch, 1, A, R, _obs(rs, arch, 1, 5), _targets(rs, A, R, 5))


def test_sample_at_head_size_limit():
    """mt_sample at A = 32, R = 31: chi-square of both heads against _draw_probs over 4 x 4096 draws
    (every category's expected count >= 256); the counters advance by one per call."""
    from test_kernels_gpu import _chi2_ok, _draw_probs, _sample
    A, R, B, K = 32, 31, 4096, 4
    rs = np.random.RandomState(3231)
    p = (0.5 * rs.dirichlet(np.ones(A)) + 0.5 / A).astype(np.float32)
    q = (0.5 * rs.dirichlet(np.ones(R)) + 0.5 / R).astype(np.float32)
    assert min(p.min(), q.min()) * B * K >= 256
    pi, rep = _d(np.tile(p, (B, 1))), _d(np.tile(q, (B, 1)))
    ctr = torch.zeros(B, dtype=torch.int64, device='cuda')
    ca, cr = np.zeros(A), np.zeros(R)
    for _ in range(K):
        a, r = _sample(pi, rep, 4321, ctr)
        ca += np.bincount(a.cpu().numpy(), minlength=A)
        cr += np.bincount(r.cpu().numpy(), minlength=R)
    assert (ctr.cpu().numpy() == K).all()
    assert ca.sum() == B * K and cr.sum() == B * K
    _chi2_ok(ca, _draw_probs(p))
    _chi2_ok(cr, _draw_probs(q))


def _launches(fn):
    """fn() under a launch window: the number of loss-kernel / grouped launches it issued."""
    from manette_amd import _lib
    lib = _lib.hip()
    lib.mt_launch_window(0, -1)
    try:
        fn()
    finally:
        seen = lib.mt_launch_window(-1, -1)
    return seen


@pytest.mark.parametrize('bad,match', [(dict(A=33), 'num_actions'), (dict(R=32), 'num_reps'), (dict(A=0), 'num_actions'),
                                       (dict(temp=0.0), 'softmax_temp')])
def test_rejected_net_configs(bad, match):
    """One past each limit mt_net_create accepts: an MTError naming the field, nothing launched."""
    from manette_amd import _lib
    from test_kernels_gpu import _net
    kw = dict(A=6, R=11, temp=1.0)
    kw.update(bad)

    def create():
        with pytest.raises(_lib.MTError, match=match):
            _net('NIPS', 1, kw['A'], kw['R'], temp=kw['temp'])
    assert _launches(create) == 0


def test_rejected_scan_length():
    """T = 1025 > kMaxScan: mt_returns_loss_backward raises before the loss kernel (whose scan buffer
    holds 1,024 steps) or anything else is launched; the gradient is untouched."""
    from manette_amd import _lib
    T, E, A, R = 1025, 1, 6, 1
    net = _make('NIPS', 1, A, R, 110)
    obs = torch.zeros(T * E, 84, 84, 4, dtype=torch.uint8, device='cuda')
    z = lambda *sh: torch.zeros(*sh, device='cuda')
    zi = torch.zeros(T * E, dtype=torch.int32, device='cuda')
    net.grad.fill_(7.0)

    def call():
        with pytest.raises(_lib.MTError, match='T=1025'):
            net.returns_loss_backward(obs, T, E, z(T * E, A), z(T * E, R), z(T * E), zi, zi, z(T, E), z(T, E), z(E),
                                      0.99, z(T, E), z(T, E))
    assert _launches(call) == 0
    torch.cuda.synchronize()
    assert (net.grad == 7.0).all()


@pytest.mark.parametrize('T,E', [(300, 3), (1024, 1)])
def test_returns_long_scan(T, E):
    """mt_returns past the T = 20 of the other tests, up to the fused scan's limit: bit-exact."""
    from manette_amd.network import returns as dev_returns
    rs = np.random.RandomState(T + E)
    r = rs.choice([-1.0, 0.0, 1.0], size=(T, E)).astype(np.float32)
    m = (rs.rand(T, E) > 0.1).astype(np.float32)
    V = rs.randn(T, E).astype(np.float32)
    VT = rs.randn(E).astype(np.float32)
    y = torch.empty(T, E, device='cuda')
    adv = torch.empty(T, E, device='cuda')
    dev_returns(_d(r), _d(m), _d(V), _d(VT), 0.99, y, adv)
    y0, adv0 = returns.nstep_returns(r.astype(np.float64), m.astype(np.float64), V.astype(np.float64), VT, 0.99)
    np.testing.assert_array_equal(y.cpu().numpy(), y0.astype(np.float32))
    np.testing.assert_array_equal(adv.cpu().numpy(), adv0.astype(np.float32))


@pytest.mark.parametrize('T,E', [(256, 1), (257, 1), (300, 2)])
def test_fused_scan_past_256_steps(T, E):
    """The fused n-step scan at T >= 256: threads 0..255 bring in their step's reward and mask, and
    row_return's second loop (k = threadIdx.x + 256, ...) loads the rest — never run at the T = 3, 5
    of the other tests. T = 256: the loop's bound (no trip), 257: one element, 300 x 2: E > 1
    strides. Rewards / masks in pinned memory, ~10 % zero masks. == mt_returns + mt_loss_backward bit
    for bit (y, adv, loss terms, gradient), and y, adv == the oracle's scan."""
    A, R = 6, 1
    N = T * E
    net = _make('NIPS', 1, A, R, 120)
    rs = np.random.RandomState(T * 10 + E)
    obs_d = _d(_obs(rs, 'NIPS', 1, N))
    v, pi, rep = [t.clone() for t in net.forward(obs_d)]
    a_idx, r_idx = _d(rs.randint(0, A, N).astype(np.int32)), _d(rs.randint(0, R, N).astype(np.int32))
    rm, rm_dev = _pinned_rewards(rs, T, E, 0.1)
    VT = rs.randn(E).astype(np.float32)
    ref = _unfused(net, obs_d, T, E, pi, rep, v, a_idx, r_idx, rm_dev, _d(VT), 0.99)
    got = _fused(net, obs_d, T, E, pi, rep, v, a_idx, r_idx, rm_dev, _d(VT), 0.99)
    _same(ref, got)
    y0, adv0 = returns.nstep_returns(rm[0].numpy().astype(np.float64), rm[1].numpy().astype(np.float64),
                                     v.cpu().numpy().reshape(T, E).astype(np.float64), VT, 0.99)
    np.testing.assert_array_equal(got[0].cpu().numpy(), y0.astype(np.float32))
    np.testing.assert_array_equal(got[1].cpu().numpy(), adv0.astype(np.float32))
    assert 0 < int((rm[1] == 0).sum()) < N // 4
    assert got[3].abs().sum().item() > 0


# ---------------------------------------------------------------------------------------------------
# 6. exports without a test of their own
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('depth', [1, 3])
def test_preprocess_frames_bit_exact(depth):
    """mt_preprocess_frames — the in-place mode of rollout.hip / paac.py: each push's two screens
    read where the emulators left them, frame f of push j of env e = screen frame_idx[e][2 j + f] of
    a pinned bank of 40 whole 210-row screens (scattered, partly repeated). Bit-exact against
    pool_and_resize + stack_update; the entries of frame_idx past an env's push count are -1: never
    read as an index (a read of screen -1 would land before the bank)."""
    from manette_amd.network import host_device_pointer, preprocess_frames
    rs = np.random.RandomState(200 + depth)
    E, S = 7, 40
    counts = np.array([1, 4, 2, 3, 1, 4, 2], np.int32)
    bank = torch.zeros(S, 210, 160, depth, dtype=torch.uint8).pin_memory()
    bank.numpy()[...] = rs.randint(0, 256, size=bank.shape).astype(np.uint8)
    idx = np.full((E, 8), -1, np.int32)
    for e in range(E):
        idx[e, :2 * counts[e]] = rs.randint(0, S, size=2 * counts[e])
    idx[1, 2:4] = idx[1, 0:2]   # a push repeated inside an env
    idx[3, 0] = idx[3, 1]       # both frames of a push the same screen
    idx[5, :8] = idx[1, :8]     # two envs on the same screens
    used = np.arange(8)[None, :] < 2 * counts[:, None]
    assert ((idx >= 0) & (idx < S))[used].all() and (idx[~used] == -1).all() and (~used).any()
    prev = rs.randint(0, 256, size=(E, 84, 84, 4 * depth)).astype(np.uint8)
    out = torch.zeros(E, 84, 84, 4 * depth, dtype=torch.uint8, device='cuda')
    preprocess_frames(host_device_pointer(bank), _d(idx), _d(counts), E, depth,
                      _d(preprocess.ROW_LUT.astype(np.int32)), _d(preprocess.COL_LUT.astype(np.int32)), _d(prev), out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    b = bank.numpy()
    for e in range(E):
        pushes = [preprocess.pool_and_resize(b[idx[e, 2 * j]], b[idx[e, 2 * j + 1]]) for j in range(counts[e])]
        np.testing.assert_array_equal(got[e], preprocess.stack_update(prev[e], pushes, depth), err_msg='env %d' % e)


def _slab_sum_order(parts):
    """The fp32 sum of parts [S][n] in mt_sum_slabs' order (include/manette_hip.h; jobs.h
    sum_slabs_body): n a multiple of 4 — each of 16 subsets adds its slabs z = k, k + 16, ... in slab
    order from 0, then the subset sums are added s_0 + s_1 + ... + s_15 (plain slab order up to 16
    slabs); else plain slab order."""
    S, n = parts.shape
    if n % 4:
        acc = np.zeros(n, np.float32)
        for z in range(S):
            acc = acc + parts[z]
        return acc
    subs = []
    for k in range(16):
        acc = np.zeros(n, np.float32)
        for z in range(k, S, 16):
            acc = acc + parts[z]
        subs.append(acc)
    t = subs[0]
    for k in range(1, 16):
        t = t + subs[k]
    return t


# n: 1001 odd (slabs off the 16-byte grid); 60 below one block (16 float4 columns = 64 floats); 4164 =
# 65 blocks + 4 floats, the last block one live column; 4099 several blocks and a tail of 3
@pytest.mark.parametrize('n', [1001, 60, 4164, 4099])
@pytest.mark.parametrize('nslabs', [1, 9, 17])
def test_sum_slabs(nslabs, n):
    """mt_sum_slabs: out[i] = sum_z parts[z * n + i] in the promised deterministic order — bit for bit
    numpy adding in that order, and within nslabs * 2^-24 * sum |parts| of the float64 sum. nslabs 17:
    the first subset holds two slabs (past the 16 a thread batch covers, the order is not plain)."""
    from manette_amd import _lib
    rs = np.random.RandomState(nslabs * 10000 + n)
    parts = (rs.randn(nslabs, n) * np.exp(rs.uniform(-3, 3, size=(nslabs, 1)))).astype(np.float32)
    pd = _d(parts)
    out = torch.full((n + 8,), float('nan'), device='cuda')
    _lib.check(_lib.hip().mt_sum_slabs(C.c_void_p(pd.data_ptr()), nslabs, n, C.c_void_p(out.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'mt_sum_slabs')
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[n:]).all()  # nothing written past n
    got = got[:n]
    np.testing.assert_array_equal(got, _slab_sum_order(parts))
    p64 = parts.astype(np.float64)
    assert (np.abs(got - p64.sum(0)) <= nslabs * 2.0 ** -24 * np.abs(p64).sum(0)).all()
