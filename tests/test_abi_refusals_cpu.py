"""What the net entry points of the C ABI refuse, and how: (status, mt_last_error()) of calls that return
before any device work, so the library's checks — their codes, texts and order — are pinned without a
GPU. Every pointer is one small dummy buffer; only refused calls are made. Sizes in the messages come
from mt_net_workspace_bytes / mt_lstm_frames_workspace_bytes. CPU only."""
import ctypes as C

import pytest

from manette_amd import _lib

OK, ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, 1, 3, 4
ARCHS = ['NIPS', 'NATURE', 'PWYX', 'LSTM', 'BAYESIAN']
NETS = [(a, 1) for a in ARCHS] + [('NIPS', 3)]
IDS = ['%s-%d' % n for n in NETS]
SHORT = 4096  # bytes: below every workspace
B, T, E = 4, 2, 3

_buf = C.create_string_buffer(64)
X = C.cast(_buf, C.c_void_p)  # the dummy non-null pointer


@pytest.fixture(scope='module')
def lib():
    return _lib.hip()


@pytest.fixture(scope='module')
def nets(lib):
    made = {}
    for arch, depth in NETS:
        cfg = _lib.mt_net_config(_lib.MT_ARCH[arch], depth, 6, 3, 0, 0.1, 1.0, 0.5)
        h = C.c_void_p()
        _lib.check(lib.mt_net_create(C.byref(cfg), C.byref(h)))
        made[(arch, depth)] = h
    yield made
    for h in made.values():
        lib.mt_net_destroy(h)


def err(lib):
    return lib.mt_last_error().decode()


def ws_bytes(lib, net, batch):
    n = C.c_size_t()
    _lib.check(lib.mt_net_workspace_bytes(net, batch, C.byref(n)))
    return n.value


def short_msg(need):
    return 'workspace %d < %d bytes' % (SHORT, need)


# ---- the calls, every pointer the dummy buffer ---------------------------------------------------
def forward(lib, name, net, batch=B, ws=SHORT, params=X):
    return getattr(lib, name)(net, params, X, batch, X, ws, X, X, X, None)


def forward_rows(lib, net, ws=SHORT):
    return lib.mt_forward_rows(net, X, X, B, X, ws, X, SHORT, 2 * B, 0, X, X, X, None)


def forward_trunk(lib, net, ws=SHORT):
    return lib.mt_forward_trunk(net, X, X, B, X, ws, None)


def trunk_stacking(lib, net, ws=SHORT):
    return lib.mt_forward_trunk_stacking(net, X, X, X, X, 1, X, B, X, ws, X, None)


def loss_backward(lib, net, batch=B, ws=SHORT, params=X):
    return lib.mt_loss_backward(net, params, X, batch, X, ws, X, X, X, X, X, X, X, 0.02, X, X, None)


def dropout_redraw(lib, net, ws=SHORT):
    return lib.mt_dropout_redraw(net, X, B, X, ws, X, X, X, None)


def dropout_returns(lib, net, t=T, ws=SHORT):
    return lib.mt_dropout_returns_loss_backward(net, X, X, t, E, X, ws, X, X, X, X, X, X, 0.99, X, X, X, X, X, 0.02,
                                                X, X, X, None)


def returns(lib, net, t=T, ws=SHORT):
    return lib.mt_returns_loss_backward(net, X, X, t, E, X, ws, X, X, X, X, X, X, X, X, 0.99, X, X, 0.02, X, X, X,
                                        None)


def returns_boot(lib, net, t=T, ws=SHORT, boot_ws=SHORT):
    return lib.mt_returns_loss_backward_boot(net, X, X, t, E, X, ws, X, X, X, X, X, X, X, X, boot_ws, X, 0.99, X, X,
                                             0.02, X, X, X, None)


def lstm_calls(lib, net, ws=SHORT):
    """Every frame-store entry point, by name."""
    n = C.c_size_t()
    return {
        'mt_lstm_frames_workspace_bytes': lambda: lib.mt_lstm_frames_workspace_bytes(net, E, T, C.byref(n)),
        'mt_lstm_frames_forward': lambda: lib.mt_lstm_frames_forward(net, X, X, 0, 1, E, T, X, ws, None),
        'mt_lstm_windows_forward': lambda: lib.mt_lstm_windows_forward(net, X, X, 0, E, T, X, ws, X, X, X, None),
        'mt_lstm_step_forward': lambda: lib.mt_lstm_step_forward(net, X, X, 0, E, T, X, X, X, ws, X, X, X, None),
        'mt_lstm_frames_backward': lambda: lib.mt_lstm_frames_backward(net, X, X, X, E, T, X, ws, X, X, X, X, X, X, X,
                                                                       0.02, X, X, X, None),
    }


# ---- short workspaces ----------------------------------------------------------------------------
@pytest.mark.parametrize('key', NETS, ids=IDS)
@pytest.mark.parametrize('name', ['mt_forward', 'mt_forward_infer'])
def test_forward_short_workspace(lib, nets, key, name):
    net = nets[key]
    assert (forward(lib, name, net), err(lib)) == (ERR_WORKSPACE, short_msg(ws_bytes(lib, net, B)))


@pytest.mark.parametrize('key', NETS, ids=IDS)
def test_forward_rows_trunk_loss_short_workspace(lib, nets, key):
    net = nets[key]
    want = (ERR_WORKSPACE, short_msg(ws_bytes(lib, net, B)))
    assert (forward_rows(lib, net), err(lib)) == want
    assert (forward_trunk(lib, net), err(lib)) == want
    # BAYESIAN and LSTM included: the size check fires before the arch refusal
    assert (trunk_stacking(lib, net), err(lib)) == want
    assert (loss_backward(lib, net), err(lib)) == want


def test_dropout_short_workspace(lib, nets):
    net = nets[('BAYESIAN', 1)]
    assert (dropout_redraw(lib, net), err(lib)) == (ERR_WORKSPACE, short_msg(ws_bytes(lib, net, B)))
    assert (dropout_returns(lib, net), err(lib)) == (ERR_WORKSPACE, short_msg(ws_bytes(lib, net, T * E)))


@pytest.mark.parametrize('key', [k for k in NETS if k[0] not in ('LSTM', 'BAYESIAN')],
                         ids=[i for i, k in zip(IDS, NETS) if k[0] not in ('LSTM', 'BAYESIAN')])
def test_returns_short_workspace(lib, nets, key):
    net = nets[key]
    need, need_boot = ws_bytes(lib, net, T * E), ws_bytes(lib, net, E)
    assert (returns(lib, net), err(lib)) == (ERR_WORKSPACE, short_msg(need))
    pair = 'workspace %d / bootstrap workspace %d < %d / %d bytes'
    assert (returns_boot(lib, net), err(lib)) == (ERR_WORKSPACE, pair % (SHORT, SHORT, need, need_boot))
    # either workspace alone is enough to refuse
    assert (returns_boot(lib, net, ws=need), err(lib)) == (ERR_WORKSPACE, pair % (need, SHORT, need, need_boot))
    assert (returns_boot(lib, net, boot_ws=need_boot), err(lib)) == \
        (ERR_WORKSPACE, pair % (SHORT, need_boot, need, need_boot))


def test_lstm_frame_store_short_workspace(lib, nets):
    net = nets[('LSTM', 1)]
    n = C.c_size_t()
    _lib.check(lib.mt_lstm_frames_workspace_bytes(net, E, T, C.byref(n)))
    assert n.value > SHORT
    for name, call in lstm_calls(lib, net).items():
        if name != 'mt_lstm_frames_workspace_bytes':
            assert (call(), err(lib)) == (ERR_WORKSPACE, short_msg(n.value)), name


# ---- arch refusals -------------------------------------------------------------------------------
@pytest.mark.parametrize('fn,name', [(returns, 'mt_returns_loss_backward'),
                                     (returns_boot, 'mt_returns_loss_backward_boot')])
def test_returns_arch_refusals(lib, nets, fn, name):
    assert (fn(lib, nets[('LSTM', 1)]), err(lib)) == \
        (ERR_UNSUPPORTED, name + ': the LSTM arch trains through mt_lstm_frames_backward')
    assert (fn(lib, nets[('BAYESIAN', 1)]), err(lib)) == \
        (ERR_UNSUPPORTED, name + ': the BAYESIAN arch trains through mt_returns, mt_dropout_redraw and mt_loss_backward')


@pytest.mark.parametrize('arch', ['NIPS', 'NATURE', 'PWYX', 'LSTM'])
def test_dropout_calls_are_bayesian_only(lib, nets, arch):
    net = nets[(arch, 1)]
    assert (dropout_redraw(lib, net), err(lib)) == (ERR_UNSUPPORTED, 'mt_dropout_redraw: the BAYESIAN arch only')
    assert (dropout_returns(lib, net), err(lib)) == \
        (ERR_UNSUPPORTED, 'mt_dropout_returns_loss_backward: the BAYESIAN arch only')


def test_backward_bucket_launches(lib, nets):
    n = C.c_int(-1)
    for key in [('NIPS', 1), ('NATURE', 1), ('PWYX', 1), ('NIPS', 3)]:
        n.value = -1
        assert lib.mt_net_backward_bucket_launches(nets[key], C.byref(n)) == OK
        assert n.value == 2
    assert (lib.mt_net_backward_bucket_launches(nets[('LSTM', 1)], C.byref(n)), err(lib)) == \
        (ERR_UNSUPPORTED, 'the LSTM backward is not bucketed')
    assert (lib.mt_net_backward_bucket_launches(nets[('BAYESIAN', 1)], C.byref(n)), err(lib)) == \
        (ERR_UNSUPPORTED, 'the BAYESIAN backward is not bucketed (its dense gradients complete one launch later)')


@pytest.mark.parametrize('key', [k for k in NETS if k[0] != 'LSTM'], ids=[i for i, k in zip(IDS, NETS) if k[0] != 'LSTM'])
def test_frame_store_calls_need_lstm(lib, nets, key):
    # an argument error (status 1), not MT_ERR_UNSUPPORTED
    for name, call in lstm_calls(lib, nets[key]).items():
        assert (call(), err(lib)) == (ERR_ARG, 'frame-store calls need the LSTM arch'), name


def test_trunk_stacking_arch_refusals(lib, nets):
    # (a sufficient size, never a workspace: both archs refuse the call)
    net = nets[('LSTM', 1)]
    assert (trunk_stacking(lib, net, ws=ws_bytes(lib, net, B)), err(lib)) == \
        (ERR_UNSUPPORTED,
         'stacking trunk: the NIPS, gray NATURE and PWYX archs (the LSTM steps: mt_lstm_step_forward)')
    net = nets[('BAYESIAN', 1)]
    assert (trunk_stacking(lib, net, ws=ws_bytes(lib, net, B)), err(lib)) == \
        (ERR_UNSUPPORTED,
         'stacking trunk: not built for the BAYESIAN arch (call mt_forward_infer on the stacked state)')


def region(lib, net, layout, kind, layer=0):
    off, n = C.c_size_t(), C.c_size_t()
    return lib.mt_net_workspace_region(net, layout, B, T, kind, layer, C.byref(off), C.byref(n))


def test_workspace_region_refusals(lib, nets):
    assert (region(lib, nets[('LSTM', 1)], 0, 0), err(lib)) == (ERR_ARG, 'layout 0 is the non-LSTM workspace')
    for key in NETS:
        if key[0] == 'LSTM':
            continue
        net = nets[key]
        for layout in (1, 2):
            assert (region(lib, net, layout, 0), err(lib)) == (ERR_ARG, 'layouts 1 and 2 are LSTM workspaces'), key
        assert (region(lib, net, 0, 0, layer=9), err(lib)) == (ERR_ARG, 'no conv layer 9'), key
        if key[0] != 'PWYX':  # (PWYX pools conv1: it has the argmax bytes)
            assert (region(lib, net, 0, 1), err(lib)) == (ERR_ARG, 'conv layer 0 has no region of kind 1'), key
        if key[0] != 'BAYESIAN':
            for kind in (5, 6, 7):
                assert (region(lib, net, 0, kind), err(lib)) == (ERR_ARG, 'regions 5-7 belong to the BAYESIAN arch'), key
    for layout in (1, 2):
        assert (region(lib, nets[('LSTM', 1)], layout, 0, layer=9), err(lib)) == (ERR_ARG, 'no conv layer 9')
    assert (region(lib, nets[('NIPS', 1)], 3, 0), err(lib)) == (ERR_ARG, 'layout 3')


def test_net_create_refuses_an_unknown_arch(lib):
    cfg = _lib.mt_net_config(9, 1, 6, 3, 0, 0.1, 1.0, 0.5)
    h = C.c_void_p()
    assert (lib.mt_net_create(C.byref(cfg), C.byref(h)), err(lib)) == \
        (ERR_UNSUPPORTED, 'arch 9 not built into this library')
    assert not h.value


# ---- argument validation -------------------------------------------------------------------------
def test_scan_length_limit(lib, nets):
    for fn, key in [(returns, ('NIPS', 1)), (returns_boot, ('NATURE', 1)), (dropout_returns, ('BAYESIAN', 1)),
                    (returns, ('LSTM', 1)), (dropout_returns, ('PWYX', 1))]:  # (ahead of the arch refusals)
        assert fn(lib, nets[key], t=1025) == ERR_ARG
        assert err(lib) == 'T=1025 (<= 1024) and E=%d must be >= 1' % E


@pytest.mark.parametrize('key', NETS, ids=IDS)
def test_batch_and_null_arguments(lib, nets, key):
    net = nets[key]
    assert (forward(lib, 'mt_forward', net, batch=0), err(lib)) == (ERR_ARG, 'batch must be >= 1')
    assert (forward(lib, 'mt_forward', net, params=None), err(lib)) == (ERR_ARG, 'null argument')
    assert (loss_backward(lib, net, batch=0), err(lib)) == (ERR_ARG, 'batch must be >= 1')
    assert (loss_backward(lib, net, params=None), err(lib)) == (ERR_ARG, 'null argument')
    # a null argument is refused before the batch is looked at
    assert (loss_backward(lib, net, batch=0, params=None), err(lib)) == (ERR_ARG, 'null argument')
