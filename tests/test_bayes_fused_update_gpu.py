"""mt_dropout_returns_loss_backward (BAYESIAN: redraw + n-step scan + loss + backward in one call) pinned
to the three-call sequence mt_returns -> mt_dropout_redraw -> mt_loss_backward, bit for bit: two nets
with identical parameters run the same mt_forward_rows into their train workspaces under the same
dropout state; net 1 runs the three calls, net 2 the new one. Also the norm partials, the counters and
the mask stream, and the refusals (the new call on a NIPS net, MT_ROLLOUT_DROPOUT's argument checks)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import optim

pytestmark = pytest.mark.gpu

SEED, ROW0 = 0x5DEECE66D, 1000          # the rollout (E-row) workspace's stream
TSEED, TROW0 = 0x2545F4914F6CDD1D, 7000  # the train workspace's


def _net(arch, depth, A, R, keep, seed=0):
    from manette_amd.network import DeviceNetwork
    conf = dict(arch=arch, rgb=depth == 3, num_actions=A, nb_choices=R, softmax_temp=1.0,
                entropy_regularisation_strength=0.02, clip_norm=3.0, clip_norm_type='global',
                activation='relu', alpha_leaky_relu=0.1, keep_percentage=keep)
    net = DeviceNetwork(conf)
    net.init_params(seed)
    return net


def _host_masks(B, counter, keep, seed=TSEED, row0=TROW0):
    from manette_amd import _lib
    out = np.zeros((B, 256), np.uint8)
    for b in range(B):
        _lib.check(_lib.hip().mt_dropout_mask_host(seed, row0 + b, counter, keep, out[b].ctypes.data_as(C.c_void_p)))
    return out


def _rollout(net, obs, boot, T, E, A, R):
    """T mt_forward_rows into the train workspace + the bootstrap forward, as the learner's Python step."""
    N = T * E
    net.set_dropout_state('roll', SEED, ROW0, batch=E)
    tws = net.workspace(N, 'train')
    tws.zero_()
    net.set_dropout_state(tws, TSEED, TROW0, batch=N)
    values = torch.zeros(T, E, device='cuda')
    pi = torch.zeros(T, E, A, device='cuda')
    rep = torch.zeros(T, E, R, device='cuda')
    for t in range(T):
        net.forward_rows(obs[t * E:(t + 1) * E], E, tws, N, t * E, (values[t], pi[t], rep[t]), ws_key='roll')
    v_boot = net.forward(boot, E, ws_key='roll', infer=True)[0].clone()
    return tws, values, v_boot


# (T, E, depth, A, R, keep, pinned rewards / masks)
CASES = [(1, 5, 1, 6, 1, 0.8, False),    # a one-step scan, one ragged 16-row stage tile, N < 16
         (5, 8, 1, 6, 1, 0.8, False),    # 2.5 stage tiles
         (3, 17, 1, 6, 1, 0.8, False),
         (1, 5, 1, 18, 11, 0.8, False),  # the wide heads
         (5, 8, 1, 18, 11, 0.8, False),
         (3, 17, 1, 18, 11, 0.8, False),
         (5, 8, 1, 6, 1, 1.0, False),    # keep 1: the no-mask path
         (2, 5, 3, 6, 1, 0.8, False),    # RGB
         (5, 8, 1, 6, 1, 0.8, True)]     # rewards / masks read in place from pinned host memory


@pytest.mark.parametrize('T,E,depth,A,R,keep,pinned', CASES)
def test_fused_call_equals_three_calls(T, E, depth, A, R, keep, pinned):
    from manette_amd.network import returns as dev_returns, host_device_pointer
    N = T * E
    n1 = _net('BAYESIAN', depth, A, R, keep, seed=T + E)
    n2 = _net('BAYESIAN', depth, A, R, keep, seed=99)
    n2.set_variables(n1.get_variables())
    np.testing.assert_array_equal(n1.params.cpu().numpy(), n2.params.cpu().numpy())
    rs = np.random.RandomState(1000 * T + 10 * E + A)
    obs = torch.from_numpy(rs.randint(0, 256, size=(N, 84, 84, 4 * depth)).astype(np.uint8)).cuda()
    boot = torch.from_numpy(rs.randint(0, 256, size=(E, 84, 84, 4 * depth)).astype(np.uint8)).cuda()
    a_idx = torch.from_numpy(rs.randint(0, A, N).astype(np.int32)).cuda()
    r_idx = torch.from_numpy(rs.randint(0, R, N).astype(np.int32)).cuda()
    rm = torch.zeros(2, T, E, dtype=torch.float32)
    rm[0] = torch.from_numpy(rs.choice([-1.0, 0.0, 1.0], size=(T, E)).astype(np.float32))
    rm[1] = 1.0
    rm[1, T // 2, E // 2] = 0.0  # an episode end in the middle of the rollout (T = 1: at its only step)
    rm[1, T - 1, 0] = 0.0        # ... and one at the last step: V(s_T) masked out
    if pinned:
        rm = rm.pin_memory()
        rew = host_device_pointer(rm)
        msk = rew + 4 * N
    else:
        rm_d = rm.cuda()
        rew, msk = rm_d[0], rm_d[1]
    new = lambda *s: torch.full(s, float('nan'), device='cuda')
    tws1, val1, vb1 = _rollout(n1, obs, boot, T, E, A, R)
    tws2, val2, vb2 = _rollout(n2, obs, boot, T, E, A, R)
    # net 1: mt_returns -> mt_dropout_redraw -> mt_loss_backward
    y1, adv1, lt1 = new(T, E), new(T, E), new(N, 4)
    out1 = (new(N), new(N, A), new(N, R))
    dev_returns(rew, msk, val1, vb1, 0.99, y1, adv1)
    n1.dropout_redraw(N, out1, ws_key='train')
    n1.loss_backward(obs, N, out1[0], out1[1], out1[2], a_idx, r_idx, y1.view(N), adv1.view(N), loss_terms=lt1,
                     ws_key='train')
    # net 2: the one call
    y2, adv2, lt2 = new(T, E), new(T, E), new(N, 4)
    out2 = (new(N), new(N, A), new(N, R))
    n2.partials.fill_(float('nan'))
    n2.dropout_returns_loss_backward(obs, T, E, val2, a_idx, r_idx, rew, msk, vb2, 0.99, out2, y2, adv2,
                                     loss_terms=lt2, ws_key='train', norm_partials=True)
    torch.cuda.synchronize()
    c = lambda t: t.cpu().numpy()
    np.testing.assert_array_equal(c(val1), c(val2), err_msg='rollout values')
    # the redrawn v' differs from the rollout's value behind adv (else the test would not tell them apart)
    if keep < 1.0:
        assert (c(out2[0]) != c(val2).reshape(N)).any()
    for a, b, k in ((y1, y2, 'y'), (adv1, adv2, 'adv'), (out1[0], out2[0], "v'"), (out1[1], out2[1], "pi'"),
                    (out1[2], out2[2], "rep'"), (lt1, lt2, 'loss_terms'), (n1.grad, n2.grad, 'grad')):
        assert np.isfinite(c(b)).all(), k
        np.testing.assert_array_equal(c(a), c(b), err_msg=k)
    m1, m2 = n1.dropout_mask(tws1, N), n2.dropout_mask(tws2, N)
    np.testing.assert_array_equal(m1, m2, err_msg='mask bytes')
    g1, g2 = n1.get_variables('grad'), n2.get_variables('grad')
    assert set(g1) == set(g2)
    for k in g1:
        np.testing.assert_array_equal(g1[k], g2[k], err_msg=k)
        # (R = 1: the repetition head's softmax gradient is exactly zero)
        assert np.any(g2[k] != 0) or (R == 1 and 'epetition' in k), k
    # the norm partials of the backward's last launch: the project's norm tolerance against fp64
    norm = float(np.sqrt(n2.partials.double().sum().item()))
    ref = optim.global_norm([c(n2.grad)])
    assert abs(norm - ref) <= 1e-5 * ref, (norm, ref)
    # counters: each train row advanced by exactly one; the mask is the host restatement's at counter 0
    seed, row0, cnt = n2.dropout_state(tws2, N)
    assert (seed, row0) == (TSEED, TROW0) and len(cnt) == N and (cnt == 1).all()
    np.testing.assert_array_equal(m2, _host_masks(N, 0, keep))
    # a second call draws the next mask
    n2.dropout_returns_loss_backward(obs, T, E, val2, a_idx, r_idx, rew, msk, vb2, 0.99, out2, y2, adv2,
                                     loss_terms=lt2, ws_key='train', norm_partials=True)
    torch.cuda.synchronize()
    m3 = n2.dropout_mask(tws2, N)
    np.testing.assert_array_equal(m3, _host_masks(N, 1, keep))
    assert (n2.dropout_state(tws2, N)[2] == 2).all()
    if keep < 1.0:
        assert (m3 != m2).any()
    else:
        assert m2.all() and m3.all()
    np.testing.assert_array_equal(c(y2), c(y1))  # (the scan does not depend on the mask)


def test_refusals():
    from manette_amd import _lib
    from manette_amd._lib import mt_rollout_buffers
    lib = _lib.hip()
    nips = _net('NIPS', 1, 6, 1, 0.9)
    bayes = _net('BAYESIAN', 1, 6, 1, 0.9)
    T, E = 2, 4
    ws = nips.workspace(T * E)
    buf = torch.zeros(1 << 16, dtype=torch.float32, device='cuda')
    p = C.c_void_p(buf.data_ptr())
    nips.grad.fill_(7.0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # the new call on a NIPS net: MT_ERR_UNSUPPORTED, nothing launched
    rc = lib.mt_dropout_returns_loss_backward(nips._h, C.c_void_p(nips.params.data_ptr()), p, T, E,
                                              C.c_void_p(ws.data_ptr()), ws.numel(), p, p, p, p, p, p, 0.99, p, p, p, p, p,
                                              0.02, C.c_void_p(nips.grad.data_ptr()), None, None, s)
    assert rc == 3 and b'BAYESIAN' in lib.mt_last_error()
    h = C.c_void_p()
    # MT_ROLLOUT_DROPOUT with MT_ROLLOUT_BOOT_SLABS: MT_ERR_ARG with a message
    b = mt_rollout_buffers()
    b.flags = (_lib.MT_ROLLOUT_DROPOUT | _lib.MT_ROLLOUT_BOOT_SLABS | _lib.MT_ROLLOUT_PIPELINED |
               _lib.MT_ROLLOUT_ZERO_COPY)
    rc = lib.mt_rollout_create(bayes._h, E, T, p, p, C.byref(b), 0, C.byref(h))
    assert rc == 1 and b'BOOT_SLABS' in lib.mt_last_error() and not h.value
    # the bit on a NIPS net: MT_ERR_ARG
    b = mt_rollout_buffers()
    b.flags = _lib.MT_ROLLOUT_DROPOUT
    rc = lib.mt_rollout_create(nips._h, E, T, p, p, C.byref(b), 0, C.byref(h))
    assert rc == 1 and b'MT_ROLLOUT_DROPOUT' in lib.mt_last_error() and not h.value
    # a BAYESIAN net without the bit: today's refusal
    rc = lib.mt_rollout_create(bayes._h, E, T, p, p, C.byref(mt_rollout_buffers()), 0, C.byref(h))
    assert rc == 3 and b'BAYESIAN' in lib.mt_last_error() and not h.value
    torch.cuda.synchronize()
    assert bool((nips.grad == 7.0).all()) and not bool(buf.any())
