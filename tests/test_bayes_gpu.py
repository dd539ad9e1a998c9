"""BAYESIAN arch (networks.py:194-204) on the GPU: the dropout + fc4 stage, the redraw and the backward
through the mask against tests/bayes_ref.py (fp64) under the device's own mask, the mask itself
against mt_dropout_mask_host. Forward bounds as tests/test_e2e_gpu.py (rtol 2e-5; atol 2e-5 for v,
1e-6 for pi / rep), gradients 2e-4 relative L2 per variable and per output channel."""
import ctypes as C

import numpy as np
import pytest
import torch

import bayes_ref
import parity_util

pytestmark = pytest.mark.gpu

# (depth, A, R, activation, alpha, temp, keep): every value of every axis, not their product
CASES = [(1, 6, 1, 'relu', 0.1, 1.0, 0.9), (3, 9, 11, 'leaky_relu', 0.3, 0.5, 0.5),
         (1, 9, 11, 'relu', 0.1, 0.5, 0.5), (3, 6, 1, 'leaky_relu', 0.3, 1.0, 0.9)]
SEED, ROW0 = 0x5DEECE66D, 1000


def _net(arch, depth, A, R, act, alpha, temp, keep, seed=0):
    from manette_amd.network import DeviceNetwork
    conf = dict(arch=arch, rgb=depth == 3, num_actions=A, nb_choices=R, softmax_temp=temp,
                entropy_regularisation_strength=0.02, clip_norm=3.0, clip_norm_type='global',
                activation=act, alpha_leaky_relu=alpha, keep_percentage=keep)
    net = DeviceNetwork(conf)
    net.init_params(seed)
    return net


def _host_masks(B, counter, keep, seed=SEED, row0=ROW0):
    from manette_amd import _lib
    out = np.zeros((B, 256), np.uint8)
    for b in range(B):
        _lib.check(_lib.hip().mt_dropout_mask_host(seed, row0 + b, counter, keep,
                                                   out[b].ctypes.data_as(C.c_void_p)))
    return out


def _check_outputs(out, ref):
    v, pi, rep = (t.cpu().numpy() for t in out)
    np.testing.assert_allclose(v, ref[0], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(pi, ref[1], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(rep, ref[2], rtol=2e-5, atol=1e-6)


def _state_tail_is_zero(net, ws, B):
    """Nothing written past the B counters (a ragged tile's rows >= B): the state region's alignment
    padding is still zero."""
    from manette_amd import _lib
    o, n = C.c_size_t(), C.c_size_t()
    _lib.check(_lib.hip().mt_net_workspace_region(net._h, 0, B, 0, 7, 0, C.byref(o), C.byref(n)))
    end = o.value + n.value
    pad = ws[end:min((end + 255) // 256 * 256, ws.numel())]
    return not bool(pad.any())


@pytest.mark.parametrize('case', CASES, ids=[str(i) for i in range(len(CASES))])
@pytest.mark.parametrize('B', [1, 16, 17, 33])
def test_forward_mask_and_trunk_identity(case, B):
    depth, A, R, act, alpha, temp, keep = case
    net = _net('BAYESIAN', depth, A, R, act, alpha, temp, keep, seed=B)
    nips = _net('NIPS', depth, A, R, act, alpha, temp, keep)
    P = net.get_variables()
    nips.set_variables(P)  # the same conv / fc3 / head values (fc4 has no NIPS counterpart)
    rs = np.random.RandomState(10 + B)
    obs = rs.randint(0, 256, size=(B, 84, 84, 4 * depth)).astype(np.uint8)
    obs_d = torch.from_numpy(obs).cuda()
    for infer in (False, True):
        key = 'infer' if infer else 'fwd'
        net.set_dropout_state(key, SEED, ROW0, batch=B)
        ws = net.workspace(B, key)
        nips.forward(obs_d, infer=infer, ws_key=key)
        H_nips = nips.forward_branches(nips.workspace(B, key), 0, B)['H']
        for call in (0, 1):
            out = [t.clone() for t in net.forward(obs_d, infer=infer, ws_key=key)]
            torch.cuda.synchronize()
            dev = net.forward_branches(ws, 0, B)
            # the mask is the host restatement's at this call's counter; every counter advanced by one
            np.testing.assert_array_equal(dev['mask'], _host_masks(B, call, keep))
            np.testing.assert_array_equal(net.dropout_mask(ws, B), dev['mask'])
            seed, row0, counters = net.dropout_state(ws, B)
            assert (seed, row0) == (SEED, ROW0) and (counters == call + 1).all() and len(counters) == B
            assert _state_tail_is_zero(net, ws, B)
            # H3 is the NIPS net's H, bit for bit
            assert dev['H3'].tobytes() == H_nips.tobytes()
            ref = bayes_ref.forward(P, obs, dev['mask'], keep, depth, A, R, act, alpha, temp)
            _check_outputs(out, ref)
            np.testing.assert_allclose(dev['H'], ref[3]['H4'], rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize('B', [1, 17])
def test_keep_one_is_no_dropout(B):
    depth, A, R, act, alpha, temp = 1, 6, 1, 'relu', 0.1, 1.0
    net = _net('BAYESIAN', depth, A, R, act, alpha, temp, 1.0, seed=3)
    rs = np.random.RandomState(B)
    obs = rs.randint(0, 256, size=(B, 84, 84, 4)).astype(np.uint8)
    net.set_dropout_state('k1', SEED, ROW0, batch=B)
    out = net.forward(torch.from_numpy(obs).cuda(), ws_key='k1')
    torch.cuda.synchronize()
    assert net.dropout_mask(net.workspace(B, 'k1'), B).all()
    ref = bayes_ref.forward(net.get_variables(), obs, None, 1, depth, A, R, act, alpha, temp)
    assert ref[3]['D'] is ref[3]['H3']
    _check_outputs(out, ref)


def test_forward_rows_lands_in_the_train_rows():
    depth, A, R, act, alpha, temp, keep = CASES[0]
    E, N, r0 = 8, 40, 16
    net = _net('BAYESIAN', depth, A, R, act, alpha, temp, keep, seed=5)
    rs = np.random.RandomState(8)
    obs = rs.randint(0, 256, size=(E, 84, 84, 4)).astype(np.uint8)
    obs_d = torch.from_numpy(obs).cuda()
    net.set_dropout_state('alone', SEED, ROW0, batch=E)
    net.forward(obs_d, infer=True, ws_key='alone')
    alone = net.forward_branches(net.workspace(E, 'alone'), 0, E)
    tws = net.workspace(N, 'train')
    tws.zero_()
    net.set_dropout_state('roll', SEED, ROW0, batch=E)
    out = net.forward_rows(obs_d, E, tws, N, r0, net.outputs(E, 'roll'), ws_key='roll')
    torch.cuda.synchronize()
    tr = net.forward_branches(tws, 0, N)
    rows = np.arange(r0, r0 + E)
    others = np.setdiff1d(np.arange(N), rows)
    assert tr['H3'][rows].tobytes() == alone['H3'].tobytes()
    np.testing.assert_array_equal(tr['mask'][rows], _host_masks(E, 0, keep))  # the E-row workspace's state
    for k in ('H3', 'mask', 'H'):
        assert not tr[k][others].any(), k
    assert (net.dropout_state(net.workspace(E, 'roll'), E)[2] == 1).all()
    assert not net.dropout_state(tws, N)[2].any()  # the train workspace's own counters: untouched
    ref = bayes_ref.forward(net.get_variables(), obs, tr['mask'][rows], keep, depth, A, R, act, alpha, temp)
    _check_outputs(out, ref)
    np.testing.assert_allclose(tr['H'][rows], ref[3]['H4'], rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize('case', CASES[:2], ids=['0', '1'])
@pytest.mark.parametrize('B', [5, 17, 40])
def test_redraw_then_backward(case, B):
    """mt_forward, then the train step's fresh mask (mt_dropout_redraw), then mt_loss_backward with
    v' != the values behind adv: the gradient is the reference's under the SECOND mask."""
    depth, A, R, act, alpha, temp, keep = case
    net = _net('BAYESIAN', depth, A, R, act, alpha, temp, keep, seed=7 + B)
    P = net.get_variables()
    rs = np.random.RandomState(100 + B)
    obs = rs.randint(0, 256, size=(B, 84, 84, 4 * depth)).astype(np.uint8)
    a_idx = rs.randint(0, A, size=B).astype(np.int32)
    r_idx = rs.randint(0, R, size=B).astype(np.int32)
    y = rs.randn(B).astype(np.float32)
    d = lambda x: torch.from_numpy(x).cuda()
    obs_d = d(obs)
    net.set_dropout_state(B, SEED, ROW0)
    ws = net.workspace(B)
    values = net.forward(obs_d)[0].clone()
    torch.cuda.synchronize()
    before = net.forward_branches(ws, 0, B)
    out2 = (torch.empty_like(values), torch.empty(B, A, device='cuda'), torch.empty(B, R, device='cuda'))
    net.dropout_redraw(B, out2)
    torch.cuda.synchronize()
    after = net.forward_branches(ws, 0, B)
    for k in ('conv1', 'conv2'):
        assert after[k][0].tobytes() == before[k][0].tobytes(), k
    assert after['H3'].tobytes() == before['H3'].tobytes()
    np.testing.assert_array_equal(before['mask'], _host_masks(B, 0, keep))
    np.testing.assert_array_equal(after['mask'], _host_masks(B, 1, keep))
    assert (after['mask'] != before['mask']).any()
    assert (net.dropout_state(ws, B)[2] == 2).all() and _state_tail_is_zero(net, ws, B)
    ref = bayes_ref.forward(P, obs, after['mask'], keep, depth, A, R, act, alpha, temp)
    _check_outputs(out2, ref)
    assert (out2[0] != values).any()
    # the update: adv from the ROLLOUT's values, v' / pi' / rep' from the redraw
    adv = (y - values.cpu().numpy()).astype(np.float32)
    terms = torch.zeros(B, 4, device='cuda')
    net.loss_backward(obs_d, B, out2[0], out2[1], out2[2], d(a_idx), d(r_idx), d(y), d(adv), loss_terms=terms)
    torch.cuda.synchronize()
    got = net.get_variables('grad')
    br = bayes_ref.branches_checked(ref[3], after, act)
    _, G, aux = bayes_ref.loss_and_grads(P, ref[3], ref[0], ref[1], ref[2], a_idx, r_idx, y, adv, 0.02, act, alpha,
                                         temp, br=br)
    parity_util.check_grads(bayes_ref.spec(depth, A, R), got, G, set())
    np.testing.assert_allclose(terms.cpu().numpy(), aux['terms'], rtol=1e-4, atol=1e-5)
    # under the FIRST mask the reference's gradient is another one: the backward read the latest mask
    ref1 = bayes_ref.forward(P, obs, before['mask'], keep, depth, A, R, act, alpha, temp)
    _, G1, _ = bayes_ref.loss_and_grads(P, ref1[3], ref1[0], ref1[1], ref1[2], a_idx, r_idx, y, adv, 0.02, act, alpha,
                                        temp)
    assert parity_util.rel(got[bayes_ref.W4], G1[bayes_ref.W4]) > 2e-4
    # alignment padding of the flat gradient is zero
    flat = net.grad.cpu().numpy()
    pad = np.ones(net.nparams, bool)
    for _, shape, off, _ in net.vars:
        pad[off:off + int(np.prod(shape))] = False
    assert not flat[pad].any()


def test_unsupported_entry_points_refuse():
    """Status 3 (MT_ERR_UNSUPPORTED) with a message, before anything is launched: the gradient buffer
    keeps its sentinel."""
    from manette_amd import _lib
    from manette_amd._lib import mt_rollout_buffers
    depth, A, R, act, alpha, temp, keep = CASES[0]
    net = _net('BAYESIAN', depth, A, R, act, alpha, temp, keep)
    lib = _lib.hip()
    T, E = 2, 4
    ws = net.workspace(T * E)
    buf = torch.zeros(1 << 16, dtype=torch.float32, device='cuda')
    p = C.c_void_p(buf.data_ptr())
    net.grad.fill_(7.0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    wp, wn, pp, gp = C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(net.params.data_ptr()), C.c_void_p(net.grad.data_ptr())
    rc = lib.mt_returns_loss_backward(net._h, pp, p, T, E, wp, wn, p, p, p, p, p, p, p, p, 0.99, p, p, 0.02, gp, None,
                                      None, s)
    assert rc == 3 and b'mt_dropout_redraw' in lib.mt_last_error()
    rc = lib.mt_returns_loss_backward_boot(net._h, pp, p, T, E, wp, wn, p, p, p, p, p, p, p, wp, wn, p, 0.99, p, p,
                                           0.02, gp, None, None, s)
    assert rc == 3 and b'mt_dropout_redraw' in lib.mt_last_error()
    rc = lib.mt_forward_trunk_stacking(net._h, pp, p, p, p, 1, p, T * E, wp, wn, None, s)
    assert rc == 3 and b'mt_forward_infer' in lib.mt_last_error()
    h = C.c_void_p()
    rc = lib.mt_rollout_create(net._h, E, T, p, p, C.byref(mt_rollout_buffers()), 0, C.byref(h))
    assert rc == 3 and b'BAYESIAN' in lib.mt_last_error() and not h.value
    rc = lib.mt_net_backward_bucket_launches(net._h, C.byref(C.c_int()))
    assert rc == 3 and lib.mt_last_error()
    torch.cuda.synchronize()
    assert bool((net.grad == 7.0).all()) and not bool(buf.any())
