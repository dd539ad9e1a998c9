"""Scratch independence and write confinement of the net entry points (include/manette_hip.h).

Every other GPU module runs its kernels on zero-filled workspaces, a zeroed or constant gradient and
fresh outputs — the one state in which a read of a region the call did not write, or a write past a
declared size, goes unnoticed. Here every call sequence runs three times on the same inputs inside a
fresh scratch_util.Arena (every written buffer at exactly its declared size, 64 KiB of sentinel around
each): `clean` (workspaces, gradient, outputs zero), `nan` and `stale` (scratch_util.poison). After each
run the guards hold their sentinel, the gradient's padding and the hand-off counters are zero, the
inputs are unchanged and every output is finite; across the runs every output and the whole gradient
are equal bit for bit — no kernel uses a floating-point atomic and every reduction order is fixed, so
this needs no tolerance. No case waits on an unpublished env, poisons a counter or feeds an index out
of range; nothing runs twice.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import scratch_util as su
from oracle import nets

pytestmark = pytest.mark.gpu

MODES = ('clean', 'nan', 'stale')
SEED, ROW0 = 0x5DEECE66D, 1000  # the dropout stream of every BAYESIAN run


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bytes(t):
    return (t.numpy() if not t.is_cuda else t.detach().cpu().numpy()).tobytes()


class Run(object):
    """One run of a call sequence in its own arena. wss: {workspace key: (layout, a, b)} (layout 1's key is
    ('lstm_frames', E, T)), carved at exactly the size the library reports, zeroed, poisoned in the
    `nan` / `stale` modes and handed to `net` through its workspace cache; outs: {name: shape} float32
    outputs, filled with zero / NaN / stale floats; ints: {name: shape} int32 buffers the caller fills;
    net.grad and net.partials are rebound to arena views (gradient: grad_poison, padding zero)."""

    def __init__(self, net, mode, wss=(), outs=(), ints=(), seed=0):
        self.net, self.mode, self.wss = net, mode, dict(wss)
        self.rng = np.random.RandomState(977 + seed)
        sizes = {}
        for key, (layout, a, b) in self.wss.items():
            sizes[('ws', key)] = su.workspace_bytes(net, layout, a, b)
        if net is not None:
            sizes['grad'] = 4 * net.nparams
        sizes['partials'] = 4 * su._lib.MT_NORM_PARTIALS
        shapes = dict(outs)
        shapes.update(ints)
        for name, shape in shapes.items():
            sizes[name] = 4 * int(np.prod(shape))
        self.arena = su.Arena(sizes)
        pattern = 'zero' if mode == 'clean' else mode
        for key, (layout, a, b) in self.wss.items():
            ws = self.arena.buf(('ws', key))
            ws.zero_()
            if mode != 'clean':
                su.poison(ws, su.protected_regions(net, layout, a, b), mode, self.rng)
            net.adopt_workspace(key, ws)
            if net.bayesian:
                net.set_dropout_state(ws, SEED, ROW0, batch=a)
        self.t = {}
        for name, shape in dict(outs).items():
            self.t[name] = su.fill(self.arena.buf(name, torch.float32).view(*shape), pattern, self.rng)
        for name, shape in dict(ints).items():
            self.t[name] = self.arena.buf(name, torch.int32).view(*shape)
        self.t['partials'] = su.fill(self.arena.buf('partials', torch.float32), pattern, self.rng)
        if net is not None:
            net.partials = self.t['partials']
            net.grad = self.t['grad'] = self.arena.buf('grad', torch.float32)
            net.grad.zero_()
            if mode != 'clean':
                su.grad_poison(net, mode, self.rng)
        self.inputs, self.before = {}, {}

    def ws(self, key):
        return self.arena.buf(('ws', key))

    def track(self, **tensors):
        """Inputs of the sequence: byte-identical after it (finish)."""
        for name, t in tensors.items():
            self.inputs[name] = t
            self.before[name] = _bytes(t)

    def finish(self, outputs):
        """The per-run checks; returns {name: uint32 view} of the declared outputs."""
        torch.cuda.synchronize()
        self.arena.check()
        net = self.net
        for key, (layout, a, b) in self.wss.items():
            ws = self.ws(key)
            assert net._ws[key].data_ptr() == ws.data_ptr(), ('the call did not run on the arena workspace', key)
            for kind, off, n in su.protected_regions(net, layout, a, b):
                if kind == su.KIND_COUNTERS:
                    assert not bool(ws[off:off + n].any()), ('hand-off counters not zero after the launch', key)
        if net is not None:
            pad = net.grad.cpu().numpy()[~su.var_mask(net)]
            assert not pad.view(np.uint32).any(), 'alignment padding of the gradient written'
        for name, t in self.inputs.items():
            assert _bytes(t) == self.before[name], ('input changed', name)
        res = {}
        for name in outputs:
            a = self.t[name].detach().cpu().numpy()
            if a.dtype == np.float32:
                assert np.isfinite(a).all(), (self.mode, name, 'not finite', int((~np.isfinite(a)).sum()), a.size)
            res[name] = a.reshape(-1).view(np.uint32).copy()
        return res


def _where(net, name, idx):
    if name != 'grad' or net is None:
        return int(idx)
    for var, shape, off, _ in net.vars:
        if off <= idx < off + int(np.prod(shape)):
            return '%s[%d]' % (var, idx - off)
    return 'padding[%d]' % idx


def _same_bits(results, net=None):
    """Every output of the nan and stale runs == the clean run's, as uint32."""
    clean = results['clean']
    for mode in MODES[1:]:
        for name, want in clean.items():
            got = results[mode][name]
            diff = np.nonzero(got != want)[0]
            assert diff.size == 0, ('%s differs between the clean and the %s run' % (name, mode), int(diff.size),
                                    want.size, 'first at', _where(net, name, diff[0]),
                                    float(want.view(np.float32)[diff[0]]), float(got.view(np.float32)[diff[0]]))


def _three(seq, net=None):
    results = {mode: seq(mode) for mode in MODES}
    _same_bits(results, net)
    return results


def _make(arch, depth, A, R, seed, act='relu'):
    from test_kernel_axes_gpu import _make as make
    return make(arch, depth, A, R, seed, act=act)


def _obs(rs, arch, depth, B):
    from test_kernel_axes_gpu import _obs as obs
    return obs(rs, arch, depth, B)


# ---------------------------------------------------------------------------------------------------
# (a) mt_forward -> mt_loss_backward, (b) mt_forward_infer
# ---------------------------------------------------------------------------------------------------
# (NATURE 18 x 11: the head region staged in LDS). B = 1: below every tile, an odd image pair of the NIPS
# conv backward; 2: one full pair; 17: one past the 16-row dense tiles; 33: one past TileFc::BM, the
# B <= 32 forms of trunk_fused.h and dx_stream_groups' one image per block.
NETS_A = [('NIPS', 1, 6, 1, 'relu'), ('NIPS', 3, 4, 11, 'leaky_relu'), ('NATURE', 1, 18, 11, 'relu'),
          ('PWYX', 1, 4, 11, 'leaky_relu'), ('PWYX', 3, 6, 1, 'relu'), ('LSTM', 1, 9, 11, 'relu')]
IDS_A = ['%s-%d-%dx%d-%s' % n for n in NETS_A]
BATCHES = [1, 2, 17, 33]


def _oracle_parity(net, arch, depth, A, R, act, obs, tgt, ws, got):
    """tests/test_kernel_axes_gpu.py's _parity on what a run left: forward 2e-5, gradients 2e-4 per
    variable and per channel, loss terms 1e-4, the device's branches checked away from near-ties."""
    import parity_util
    from test_kernel_axes_gpu import _check_forward
    a_idx, r_idx, y, adv = tgt
    B = len(obs)
    spec = nets.arch_spec(arch, depth, A, R)
    P = net.get_variables()
    ref = nets.forward(spec, P, obs, act=act, alpha=0.1)[:3]
    _check_forward((got['v'], got['pi'], got['rep']), ref)
    if arch == 'LSTM':
        frames, dev = obs.reshape((-1,) + obs.shape[2:]), net.forward_branches(ws, 2, B)
    else:
        frames, dev = obs, net.forward_branches(ws, 0, B)
    br = parity_util.device_branches(spec, P, frames, dev, act, 0.1)
    _, G, aux = nets.loss_and_grads(spec, P, obs, a_idx, r_idx, y, adv, 0.02, act=act, alpha=0.1,
                                    routes=br['routes'], branches=br['branches'], hbranch=br['hbranch'])
    parity_util.check_grads(spec, net.get_variables('grad'), G, set())
    np.testing.assert_allclose(got['terms'].cpu().numpy(), aux['terms'], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('arch,depth,A,R,act', NETS_A, ids=IDS_A)
def test_forward_then_loss_backward(arch, depth, A, R, act, B):
    """(a). At B = 1 and 2 — the first backward runs below 3 rows — the stale run is also held against
    the float64 oracle at the project's bounds."""
    from test_kernel_axes_gpu import _targets
    net = _make(arch, depth, A, R, 300 + B, act)
    rs = np.random.RandomState(310 + B + depth)
    obs = _obs(rs, arch, depth, B)
    tgt = _targets(rs, A, R, B)
    obs_d, (a_d, r_d, y_d, adv_d) = _d(obs), [_d(x) for x in tgt]
    layout = 2 if arch == 'LSTM' else 0

    def seq(mode):
        run = Run(net, mode, {'fb': (layout, B, 0)}, dict(v=(B,), pi=(B, A), rep=(B, R), terms=(B, 4)), seed=B)
        run.track(params=net.params, obs=obs_d, a_idx=a_d, r_idx=r_d, y=y_d, adv=adv_d)
        o = run.t
        net.forward(obs_d, B, out=(o['v'], o['pi'], o['rep']), ws_key='fb')
        net.loss_backward(obs_d, B, o['v'], o['pi'], o['rep'], a_d, r_d, y_d, adv_d, loss_terms=o['terms'],
                          ws_key='fb')
        res = run.finish(['v', 'pi', 'rep', 'terms', 'grad'])
        if mode == 'stale' and B <= 2:
            _oracle_parity(net, arch, depth, A, R, act, obs, tgt, run.ws('fb'), o)
        return res
    _three(seq, net)


FUSED_CAP = 1280  # nips_bwd.h kNipsFusedBwdMaxRows


@pytest.mark.parametrize('B', [FUSED_CAP, FUSED_CAP + 1])
def test_forward_then_loss_backward_at_the_fused_cap(B):
    """(a) at the last batch of the fused NIPS conv backward — the largest per-image and per-pair slab
    regions ws_layout sizes — and at the first of the layered trunk_backward, whose slab regions are
    sized by conv_wgrad_slab alone."""
    from test_kernel_axes_gpu import _targets
    A, R = 6, 1
    net = _make('NIPS', 1, A, R, 305)
    rs = np.random.RandomState(306)
    obs_d = _d(_obs(rs, 'NIPS', 1, B))
    a_d, r_d, y_d, adv_d = [_d(x) for x in _targets(rs, A, R, B)]

    def seq(mode):
        run = Run(net, mode, {'cap': (0, B, 0)}, dict(v=(B,), pi=(B, A), rep=(B, R), terms=(B, 4)), seed=B)
        run.track(params=net.params, obs=obs_d, a_idx=a_d, r_idx=r_d, y=y_d, adv=adv_d)
        o = run.t
        net.forward(obs_d, B, out=(o['v'], o['pi'], o['rep']), ws_key='cap')
        net.loss_backward(obs_d, B, o['v'], o['pi'], o['rep'], a_d, r_d, y_d, adv_d, loss_terms=o['terms'],
                          ws_key='cap')
        return run.finish(['v', 'pi', 'rep', 'terms', 'grad'])
    _three(seq, net)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('arch,depth,A,R,act', NETS_A, ids=IDS_A)
def test_forward_infer(arch, depth, A, R, act, B):
    """(b): the inference forward (NIPS: the fused trunk and its 9 slabs)."""
    net = _make(arch, depth, A, R, 320 + B, act)
    obs_d = _d(_obs(np.random.RandomState(330 + B + depth), arch, depth, B))
    layout = 2 if arch == 'LSTM' else 0

    def seq(mode):
        run = Run(net, mode, {'inf': (layout, B, 0)}, dict(v=(B,), pi=(B, A), rep=(B, R)), seed=B)
        run.track(params=net.params, obs=obs_d)
        o = run.t
        net.forward(obs_d, B, out=(o['v'], o['pi'], o['rep']), ws_key='inf', infer=True)
        return run.finish(['v', 'pi', 'rep'])
    _three(seq, net)


# ---------------------------------------------------------------------------------------------------
# (c) mt_forward_rows x T -> mt_returns_loss_backward, (d) ... -> mt_forward_trunk -> _boot
# ---------------------------------------------------------------------------------------------------
ROLLOUTS = [(1, 1), (3, 3), (17, 2)]  # (E, T)


def _rollout_inputs(rs, arch, depth, A, R, E, T):
    N = T * E
    return dict(obs=_d(_obs(rs, arch, depth, N).reshape(T, E, 84, 84, 4 * depth)),
                a_idx=_d(rs.randint(0, A, N).astype(np.int32)), r_idx=_d(rs.randint(0, R, N).astype(np.int32)),
                rewards=_d(rs.choice([-1.0, 0.0, 1.0], size=(T, E)).astype(np.float32)),
                masks=_d((rs.rand(T, E) > 0.2).astype(np.float32)))


def _rollout_outs(E, T, A, R):
    N = T * E
    return dict(v=(T, E), pi=(T, E, A), rep=(T, E, R), y=(T, E), adv=(T, E), terms=(N, 4))


@pytest.mark.parametrize('E,T', ROLLOUTS)
@pytest.mark.parametrize('arch,A,R', [('NIPS', 6, 1), ('NATURE', 4, 11), ('PWYX', 4, 11)])
def test_forward_rows_then_returns_backward(arch, A, R, E, T):
    """(c): the rollout's T forwards into a train workspace, then the update's fused backward with the
    norm partials. The E-row and the T*E-row workspace are both poisoned before the first call. All
    MT_NORM_PARTIALS partials are compared (every form of the backward writes all of them from fixed
    grids), which covers the sum mt_clip_rmsprop takes."""
    N = T * E
    net = _make(arch, 1, A, R, 340 + E)
    rs = np.random.RandomState(350 + E + T)
    inp = _rollout_inputs(rs, arch, 1, A, R, E, T)
    v_boot = _d(rs.randn(E).astype(np.float32))

    def seq(mode):
        run = Run(net, mode, {'rows': (0, E, 0), 'train': (0, N, 0)}, _rollout_outs(E, T, A, R), seed=N)
        run.track(params=net.params, v_boot=v_boot, **inp)
        o = run.t
        for t in range(T):
            net.forward_rows(inp['obs'][t], E, run.ws('train'), N, t * E, (o['v'][t], o['pi'][t], o['rep'][t]),
                             ws_key='rows')
        net.returns_loss_backward(inp['obs'].view(N, 84, 84, 4), T, E, o['pi'], o['rep'], o['v'], inp['a_idx'],
                                  inp['r_idx'], inp['rewards'], inp['masks'], v_boot, 0.99, o['y'], o['adv'],
                                  loss_terms=o['terms'], ws_key='train', norm_partials=True)
        return run.finish(['v', 'pi', 'rep', 'y', 'adv', 'terms', 'grad', 'partials'])
    _three(seq, net)


@pytest.mark.parametrize('E,T', ROLLOUTS)
@pytest.mark.parametrize('arch,A,R', [('NIPS', 6, 1), ('NATURE', 4, 11)])
def test_forward_trunk_then_boot_backward(arch, A, R, E, T):
    """(d): the bootstrap's dense slabs left by mt_forward_trunk in an E-row workspace poisoned before
    the trunk call, finished into V(s_T) by the loss kernel of mt_returns_loss_backward_boot."""
    N = T * E
    net = _make(arch, 1, A, R, 360 + E)
    rs = np.random.RandomState(370 + E + T)
    inp = _rollout_inputs(rs, arch, 1, A, R, E, T)
    obs_T = _d(_obs(rs, arch, 1, E))

    def seq(mode):
        outs = _rollout_outs(E, T, A, R)
        outs['v_boot'] = (E,)
        run = Run(net, mode, {'rows': (0, E, 0), 'train': (0, N, 0), 'boot': (0, E, 0)}, outs, seed=N)
        run.track(params=net.params, obs_T=obs_T, **inp)
        o = run.t
        for t in range(T):
            net.forward_rows(inp['obs'][t], E, run.ws('train'), N, t * E, (o['v'][t], o['pi'][t], o['rep'][t]),
                             ws_key='rows')
        net.forward_trunk(obs_T, E, ws_key='boot')
        net.returns_loss_backward(inp['obs'].view(N, 84, 84, 4), T, E, o['pi'], o['rep'], o['v'], inp['a_idx'],
                                  inp['r_idx'], inp['rewards'], inp['masks'], o['v_boot'], 0.99, o['y'], o['adv'],
                                  loss_terms=o['terms'], ws_key='train', norm_partials=True, boot_ws=run.ws('boot'))
        return run.finish(['v', 'pi', 'rep', 'v_boot', 'y', 'adv', 'terms', 'grad', 'partials'])
    _three(seq, net)


# ---------------------------------------------------------------------------------------------------
# (e) the LSTM frame store: mt_lstm_step_forward t = 0 .. T -> mt_lstm_frames_backward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('depth,E,T', [(1, 1, 1), (1, 3, 2), (3, 2, 2)])
def test_lstm_steps_then_frames_backward(depth, E, T):
    """(e): the rollout's steps 0 .. T-1 and the bootstrap windows (step T), nz rows t > 0 derived on the
    device over pre-filled garbage in 0..5 with some episode ends, then the frames backward with the
    norm partials, on a poisoned frame-store workspace (torch.empty in production)."""
    A, R = 9, 11
    N = T * E
    from test_lstm_gpu import _net
    net = _net(depth, A, R, seed=380 + E)
    rs = np.random.RandomState(390 + E + T + depth)
    fstore = rs.randint(0, 256, size=(1 + (T + 5) * E, 84, 84, 4 * depth)).astype(np.uint8)
    fstore[0] = 0
    fs_d = _d(fstore)
    nz0 = rs.choice([0, 0, 2, 5], size=E).astype(np.int32)
    over = (rs.rand(T + 1, E) < 0.4).astype(np.float32)
    over[0, 0] = 1.0  # (step 1 of env 0 follows an episode end)
    over_d = _d(over)
    a_d, r_d = _d(rs.randint(0, A, N).astype(np.int32)), _d(rs.randint(0, R, N).astype(np.int32))
    y_d, adv_d = _d(rs.randn(N).astype(np.float32)), _d(rs.randn(N).astype(np.float32))
    key = ('lstm_frames', E, T)

    def seq(mode):
        run = Run(net, mode, {key: (1, E, T)}, dict(v=(T + 1, E), pi=(T + 1, E, A), rep=(T + 1, E, R), terms=(N, 4)),
                  ints=dict(nz=(T + 1, E)), seed=N)
        o = run.t
        o['nz'].copy_(_d(run.rng.randint(0, 6, size=(T + 1, E)).astype(np.int32) * (mode != 'clean')))
        o['nz'][0].copy_(_d(nz0))
        run.track(params=net.params, fstore=fs_d, over=over_d, a_idx=a_d, r_idx=r_d, y=y_d, adv=adv_d)
        for t in range(T + 1):
            net.lstm_step_forward(fs_d, t, E, T, o['nz'], over_d[t - 1] if t > 0 else None,
                                  out=(o['v'][t], o['pi'][t], o['rep'][t]))
        net.lstm_frames_backward(fs_d, o['nz'], E, T, o['pi'], o['rep'], o['v'], a_d, r_d, y_d, adv_d,
                                 loss_terms=o['terms'], norm_partials=True)
        res = run.finish(['v', 'pi', 'rep', 'nz', 'terms', 'grad', 'partials'])
        nz = o['nz'].cpu().numpy()
        assert (nz[0] == nz0).all()  # the caller's row
        for t in range(1, T + 1):    # the header's rule
            assert (nz[t] == np.where(over[t - 1] != 0, 5, np.maximum(nz[t - 1] - 1, 0))).all(), t
        return res
    _three(seq, net)


# ---------------------------------------------------------------------------------------------------
# (f) BAYESIAN
# ---------------------------------------------------------------------------------------------------
def _bayes(keep, seed):
    from test_bayes_gpu import _net
    return _net('BAYESIAN', 1, 6, 3, 'relu', 0.1, 1.0, keep, seed=seed)


@pytest.mark.parametrize('E,T', [(1, 1), (3, 3)])
@pytest.mark.parametrize('keep', [0.5, 1.0])
def test_bayes_rows_then_dropout_returns_backward(keep, E, T):
    """(f), the update in one call: T mt_forward_rows (masks from the E-row workspace's dropout state),
    then mt_dropout_returns_loss_backward (fresh masks from the train workspace's state). Both states
    are seeded alike in every run; each E-row counter advanced by T, each train-row counter by one."""
    A, R, N = 6, 3, T * E
    net = _bayes(keep, 400 + E)
    rs = np.random.RandomState(410 + E)
    inp = _rollout_inputs(rs, 'BAYESIAN', 1, A, R, E, T)
    v_boot = _d(rs.randn(E).astype(np.float32))

    def seq(mode):
        outs = _rollout_outs(E, T, A, R)
        outs.update(v2=(T, E), pi2=(T, E, A), rep2=(T, E, R))
        run = Run(net, mode, {'rows': (0, E, 0), 'train': (0, N, 0)}, outs, seed=N)
        run.track(params=net.params, v_boot=v_boot, **inp)
        o = run.t
        for t in range(T):
            net.forward_rows(inp['obs'][t], E, run.ws('train'), N, t * E, (o['v'][t], o['pi'][t], o['rep'][t]),
                             ws_key='rows')
        net.dropout_returns_loss_backward(inp['obs'].view(N, 84, 84, 4), T, E, o['v'], inp['a_idx'], inp['r_idx'],
                                          inp['rewards'], inp['masks'], v_boot, 0.99, (o['v2'], o['pi2'], o['rep2']),
                                          o['y'], o['adv'], loss_terms=o['terms'], ws_key='train', norm_partials=True)
        res = run.finish(['v', 'pi', 'rep', 'v2', 'pi2', 'rep2', 'y', 'adv', 'terms', 'grad', 'partials'])
        assert net.dropout_state(run.ws('rows'), E)[:2] == (SEED, ROW0)
        assert (net.dropout_state(run.ws('rows'), E)[2] == T).all()
        assert (net.dropout_state(run.ws('train'), N)[2] == 1).all()
        res['mask'] = net.dropout_mask(run.ws('train'), N).reshape(-1).astype(np.uint32)
        return res
    _three(seq, net)


@pytest.mark.parametrize('B', [1, 9])
@pytest.mark.parametrize('keep', [0.5, 1.0])
def test_bayes_forward_redraw_backward(keep, B):
    """(f), the update in three calls: mt_forward, mt_dropout_redraw, mt_loss_backward; every counter
    advanced by two."""
    from test_kernel_axes_gpu import _targets
    A, R = 6, 3
    net = _bayes(keep, 420 + B)
    rs = np.random.RandomState(430 + B)
    obs_d = _d(_obs(rs, 'BAYESIAN', 1, B))
    a_d, r_d, y_d, adv_d = [_d(x) for x in _targets(rs, A, R, B)]

    def seq(mode):
        run = Run(net, mode, {'fb': (0, B, 0)}, dict(v=(B,), pi=(B, A), rep=(B, R), v2=(B,), pi2=(B, A), rep2=(B, R),
                                                     terms=(B, 4)), seed=B)
        run.track(params=net.params, obs=obs_d, a_idx=a_d, r_idx=r_d, y=y_d, adv=adv_d)
        o = run.t
        net.forward(obs_d, B, out=(o['v'], o['pi'], o['rep']), ws_key='fb')
        net.dropout_redraw(B, (o['v2'], o['pi2'], o['rep2']), ws_key='fb')
        net.loss_backward(obs_d, B, o['v2'], o['pi2'], o['rep2'], a_d, r_d, y_d, adv_d, loss_terms=o['terms'],
                          ws_key='fb')
        res = run.finish(['v', 'pi', 'rep', 'v2', 'pi2', 'rep2', 'terms', 'grad'])
        assert (net.dropout_state(run.ws('fb'), B)[2] == 2).all()
        res['mask'] = net.dropout_mask(run.ws('fb'), B).reshape(-1).astype(np.uint32)
        return res
    _three(seq, net)


# ---------------------------------------------------------------------------------------------------
# (g) mt_forward_trunk_stacking, every ready word published
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', [1, 17])
@pytest.mark.parametrize('arch,depth', [('NIPS', 1), ('NATURE', 1), ('PWYX', 1), ('PWYX', 3)])
def test_stacking_trunk(arch, depth, E):
    """(g): the stacked state and everything the trunk leaves in the workspace. The ABI has no heads-only
    call, so the slabs are compared in place: the words the launch wrote are those of the nan run that no
    longer hold the NaN word (a trunk output is finite), the three runs agree on them bit for bit, and
    the stale run left every other scratch word as poisoned. Counters zero afterwards (Run.finish)."""
    from manette_amd.network import WaitStatus, host_device_pointer
    net = _make(arch, depth, 6, 11, 440 + E)
    rs = np.random.RandomState(450 + E + depth)
    counts = rs.randint(1, 5, E).astype(np.int32)
    counts[0] = 4
    frames = torch.zeros(4 * E, 84, 84, depth, dtype=torch.uint8).pin_memory()
    frames.numpy()[...] = rs.randint(0, 256, size=frames.shape).astype(np.uint8)
    tag = 777
    ready = torch.zeros(E, 32, dtype=torch.int32).pin_memory()  # MH_READY_STRIDE words per env
    ready.numpy()[:, 0] = (tag << 3) | counts
    prev = _d(rs.randint(0, 256, size=(E, 84, 84, 4 * depth)).astype(np.uint8))
    fdev, rdev = C.c_void_p(host_device_pointer(frames)), C.c_void_p(host_device_pointer(ready))
    status = WaitStatus()
    words, poisoned = {}, {}

    def seq(mode):
        run = Run(net, mode, {'stk': (0, E, 0)}, ints=dict(out=(E * 84 * 84 * depth,)), seed=E)
        out = run.t['out'].view(torch.uint8).view(E, 84, 84, 4 * depth)
        out.fill_(0 if mode == 'clean' else 0x7F)
        run.track(params=net.params, prev=prev, frames=frames, ready=ready)
        poisoned[mode] = run.ws('stk').cpu().numpy().view(np.uint32)
        net.forward_trunk_stacking(prev, fdev, rdev, tag, out, E, ws_key='stk', status=status)
        res = run.finish(['out'])
        status.check('stacking trunk')
        words[mode] = run.ws('stk').cpu().numpy().view(np.uint32)
        return res
    _three(seq, net)
    scratch = np.ones(words['nan'].size, bool)
    for kind, off, n in su.protected_regions(net, 0, E, 0):
        scratch[off // 4:(off + n + 3) // 4] = False
    written = scratch & (words['nan'] != su.NAN_WORD)
    assert written.any()
    assert np.isfinite(words['nan'].view(np.float32)[written]).all()
    for mode in ('clean', 'stale'):
        diff = np.nonzero(written & (words[mode] != words['nan']))[0]
        assert diff.size == 0, (mode, 'workspace words the launch wrote differ from the nan run', int(diff.size),
                                'first word', int(diff[0]))
    rest = scratch & ~written
    assert (words['stale'][rest] == poisoned['stale'][rest]).all(), 'the stale run wrote words the nan run did not'


# ---------------------------------------------------------------------------------------------------
# (h) mt_grad_sumsq -> mt_clip_rmsprop
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 63, 64, 4099])
def test_sumsq_then_clip_rmsprop(n):
    """(h): tails of the vector width and fewer elements than partials; w, ms, mom, g, the partials and
    norm_out carved from the arena, partials and norm_out poisoned."""
    lib = su._lib.hip()
    rs = np.random.RandomState(460 + n)
    g0 = (rs.randn(n) * 10).astype(np.float32)
    w0, ms0, mom0 = rs.randn(n).astype(np.float32), (1 + rs.rand(n)).astype(np.float32), \
        (rs.randn(n) * 1e-3).astype(np.float32)
    lr = _d(np.array([0.0224], np.float32))
    p = lambda t: C.c_void_p(t.data_ptr())

    def seq(mode):
        run = Run(None, mode, outs=dict(norm=(1,), w=(n,), ms=(n,), mom=(n,), g=(n,)), seed=n)
        o = run.t
        for name, a in (('w', w0), ('ms', ms0), ('mom', mom0), ('g', g0)):
            o[name].copy_(_d(a))
        run.track(g=o['g'], lr=lr)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        su._lib.check(lib.mt_grad_sumsq(p(o['g']), n, 1.0, p(o['partials']), s), 'mt_grad_sumsq')
        su._lib.check(lib.mt_clip_rmsprop(p(o['w']), p(o['ms']), p(o['mom']), p(o['g']), n, p(o['partials']), p(lr), 0.99,
                                          0.0, 0.1, 3.0, 1, 1.0, p(o['norm']), s), 'mt_clip_rmsprop')
        return run.finish(['partials', 'norm', 'w', 'ms', 'mom'])
    res = _three(seq)
    norm = float(res['clean']['norm'].view(np.float32)[0])
    ref = float(np.sqrt((g0.astype(np.float64) ** 2).sum()))
    assert abs(norm - ref) <= 1e-5 * ref, (norm, ref)  # (tests/test_kernels_gpu.py test_clip_rmsprop's bound)


# ---------------------------------------------------------------------------------------------------
# The persistent NIPS trunk's entry boundary (trunk_fused.h kPersistMinEnvs = 256, grid min(B, CUs))
# ---------------------------------------------------------------------------------------------------
_PERSIST = {}


def _persist_case():
    """257 rows, their network and the oracle's outputs (trunk in chunks of 32 rows), computed once."""
    if not _PERSIST:
        net = _make('NIPS', 1, 6, 1, 470)
        obs = np.random.RandomState(471).randint(0, 256, size=(257, 84, 84, 4)).astype(np.uint8)
        spec, P = nets.arch_spec('NIPS', 1, 6, 1), net.get_variables()
        feats = np.concatenate([nets.trunk_forward(spec, P, obs[c:c + 32])[0] for c in range(0, 257, 32)])
        _PERSIST.update(net=net, obs=_d(obs), ref=nets.heads_forward(spec, P, feats)[:3])
    return _PERSIST


@pytest.mark.parametrize('B', [255, 256, 257])
def test_persistent_trunk_entry(B):
    """B = 255: the last batch of the latency form; 256: a persistent grid in which no block walks to a
    second env; 257: one in which exactly one does. mt_forward_infer vs mt_forward on the same rows, vs
    the oracle, and bit-equal between a clean and a stale-poisoned workspace, inside an arena."""
    c = _persist_case()
    net, obs_d, A, R = c['net'], c['obs'][:B], 6, 1
    res = {}
    for mode in ('clean', 'stale'):
        run = Run(net, mode, {'inf': (0, B, 0)}, dict(v=(B,), pi=(B, A), rep=(B, R)), seed=B)
        run.track(params=net.params, obs=obs_d)
        o = run.t
        net.forward(obs_d, B, out=(o['v'], o['pi'], o['rep']), ws_key='inf', infer=True)
        res[mode] = run.finish(['v', 'pi', 'rep'])
    _same_bits({'clean': res['clean'], 'nan': res['clean'], 'stale': res['stale']}, net)
    v, pi, rep = (res['stale'][k].view(np.float32) for k in ('v', 'pi', 'rep'))
    v1, pi1, rep1 = net.forward(obs_d, B, ws_key='layered')
    torch.cuda.synchronize()
    for got, (want, atol) in zip((v, pi, rep), zip(c['ref'], (2e-5, 1e-6, 1e-6))):
        np.testing.assert_allclose(got, want[:B].reshape(-1), rtol=2e-5, atol=atol)
    np.testing.assert_allclose(v, v1.cpu().numpy(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(pi, pi1.cpu().numpy().reshape(-1), rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(rep, rep1.cpu().numpy().reshape(-1), rtol=2e-5, atol=1e-6)
