"""BAYESIAN arch (networks.py:194-204) without a GPU: the parameter layout, the keep_prob checks, the
dropout mask's host restatement against numpy and its statistics, checkpoints, the CLI."""
import ctypes as C

import numpy as np
import pytest

import bayes_ref

KEEPS = (0.5, 0.9, 1.0)


def _create(arch, depth, A, R, keep):
    from manette_amd import _lib
    lib = _lib.hip()
    cfg = _lib.mt_net_config(_lib.MT_ARCH[arch], depth, A, R, 0, 0.1, 1.0, keep)
    h = C.c_void_p()
    return lib, lib.mt_net_create(C.byref(cfg), C.byref(h)), h


def _host_mask(seed, row, counter, keep):
    from manette_amd import _lib
    out = np.zeros(256, np.uint8)
    _lib.check(_lib.hip().mt_dropout_mask_host(seed, row, counter, keep, out.ctypes.data_as(C.c_void_p)))
    return out


@pytest.mark.parametrize('depth,A,R', [(1, 6, 1), (3, 9, 11)])
def test_layout(depth, A, R):
    """Names, order, shapes, init bounds, 64-float alignment and (weights, biases) contiguity, as
    test_cpu_library.test_layout_matches_oracle checks the other archs."""
    from manette_amd import _lib
    lib, rc, h = _create('BAYESIAN', depth, A, R, 0.9)
    assert rc == 0, lib.mt_last_error()
    try:
        spec = bayes_ref.spec(depth, A, R)
        names = [n for n, _, _ in spec['vars']]
        assert names[4:8] == ['Network/fc3/fc3_weights', 'Network/fc3/fc3_biases', 'Network_1/fc4/fc4_weights',
                              'Network_1/fc4/fc4_biases'] and names[8].startswith('Training/Critic')
        nv = C.c_int()
        lib.mt_net_num_vars(h, C.byref(nv))
        assert nv.value == len(spec['vars']) == 14
        prev_end = 0
        for i, (name, shape, bound) in enumerate(spec['vars']):
            buf = C.create_string_buffer(256)
            sh = (C.c_int64 * 4)()
            nd = C.c_int()
            off = C.c_size_t()
            b = C.c_float()
            _lib.check(lib.mt_net_var_info(h, i, buf, 256, sh, C.byref(nd), C.byref(off), C.byref(b)))
            assert buf.value.decode() == name
            assert tuple(sh[k] for k in range(nd.value)) == tuple(shape)
            assert np.float32(b.value) == np.float32(bound)
            if i % 2 == 1:
                assert off.value == prev_end  # (weights, biases) contiguous
            else:
                assert off.value >= prev_end and off.value % 64 == 0
            prev_end = off.value + int(np.prod(shape))
        n = C.c_size_t()
        lib.mt_net_num_params(h, C.byref(n))
        assert n.value >= prev_end
        total = sum(int(np.prod(sh)) for _, sh, _ in spec['vars'])
        if (depth, A, R) == (1, 6, 1):
            assert total == 743992  # the NIPS net's 678,200 + fc4's 65,792
        f = C.c_int()
        _lib.check(lib.mt_net_feature_dim(h, C.byref(f)))
        assert f.value == 256
        ws = C.c_size_t()
        _lib.check(lib.mt_net_workspace_bytes(h, 160, C.byref(ws)))
        assert ws.value > 0
        # the dropout regions: inside the workspace, disjoint, sized for the rows
        spans = []
        for kind, nbytes in ((5, 160 * 256), (6, 160 * 256 * 4), (7, (2 + 160) * 8), (2, 160 * 256 * 4)):
            o, nb = C.c_size_t(), C.c_size_t()
            _lib.check(lib.mt_net_workspace_region(h, 0, 160, 0, kind, 0, C.byref(o), C.byref(nb)))
            assert nb.value == nbytes and o.value % 8 == 0 and o.value + nb.value <= ws.value
            spans.append((o.value, o.value + nb.value))
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        rc = lib.mt_net_backward_bucket_launches(h, C.byref(C.c_int()))
        assert rc == 3 and lib.mt_last_error()
    finally:
        lib.mt_net_destroy(h)


@pytest.mark.parametrize('keep', [0.0, 1.5, float('nan'), -0.5])
def test_keep_prob_is_checked(keep):
    lib, rc, h = _create('BAYESIAN', 1, 6, 1, keep)
    assert rc == 1 and b'keep_prob' in lib.mt_last_error()
    lib, rc, h = _create('NIPS', 1, 6, 1, keep)  # the other archs ignore the field
    assert rc == 0
    lib.mt_net_destroy(h)


def test_seven_value_config_still_builds():
    from manette_amd import _lib
    cfg = _lib.mt_net_config(_lib.MT_ARCH['NIPS'], 1, 6, 1, 0, 0.1, 1.0)
    assert cfg.keep_prob == 0.0
    h = C.c_void_p()
    _lib.check(_lib.hip().mt_net_create(C.byref(cfg), C.byref(h)))
    _lib.hip().mt_net_destroy(h)


def test_mask_host_equals_numpy():
    seeds = (0, 1, 0x9e3779b97f4a7c15, 2 ** 64 - 1)
    rows = (0, 1, 31, 159, 2 ** 20 + 3)
    counters = (0, 1, 2, 1000, 2 ** 40 + 7)
    for keep in KEEPS:
        for seed in seeds:
            for row in rows:
                for c in counters:
                    got = _host_mask(seed, row, c, keep)
                    assert set(np.unique(got)) <= {0, 1}
                    np.testing.assert_array_equal(got, bayes_ref.np_mask(seed, row, c, keep), err_msg=str((keep, seed, row, c)))
                    if keep == 1.0:
                        assert got.all()
    for keep in (0.5, 0.9):
        a, b, c = _host_mask(7, 3, 0, keep), _host_mask(7, 3, 1, keep), _host_mask(7, 4, 0, keep)
        assert (a != b).any() and (a != c).any() and (b != c).any()
        assert (_host_mask(8, 3, 0, keep) != a).any()


def _p_exact(keep):
    """The kept share of the 65,536 field values under the fp32 rule, by enumeration."""
    u = np.arange(65536, dtype=np.float32) * np.float32(2.0 ** -16)
    return float(((np.float32(keep) + u).astype(np.float32) >= np.float32(1.0)).mean())


@pytest.mark.parametrize('keep', [0.5, 0.9])
def test_mask_statistics(keep):
    """Fixed inputs (seed 20261, chosen on the CPU): the kept share of 2^20 bits and of each feature
    over 4,096 (row, counter) pairs within 5 sigma of the exact probability of the fp32 rule."""
    p = _p_exact(keep)
    assert abs(p - keep) <= 2.0 ** -16 + 1e-7  # (0.9f is not a multiple of 2^-16: p is the enumerated value)
    seed = 20261
    m = np.stack([_host_mask(seed, row, c, keep) for row in range(64) for c in range(64)]).astype(np.float64)
    assert m.shape == (4096, 256) and m.size == 2 ** 20
    sig = np.sqrt(p * (1 - p))
    assert abs(m.mean() - p) <= 5 * sig / np.sqrt(m.size), (m.mean(), p)
    per = m.mean(axis=0)
    assert (np.abs(per - p) <= 5 * sig / np.sqrt(4096)).all(), (float(np.abs(per - p).max()), 5 * sig / 64)


def test_bundle_round_trip_of_bayesian_variables(tmp_path):
    from manette_amd import tf_bundle
    rs = np.random.RandomState(3)
    t = {n: rs.randn(*shape).astype(np.float32) for n, shape, _ in bayes_ref.spec(1, 6, 1)['vars']}
    assert 'Network_1/fc4/fc4_weights' in t and 'Network_1/fc4/fc4_biases' in t
    pre = str(tmp_path / '-7')
    tf_bundle.write_bundle(pre, t)
    back = tf_bundle.read_bundle(pre)
    assert set(back) == set(t)
    for k in t:
        np.testing.assert_array_equal(back[k], t[k])


def test_cli_carries_keep_percentage_and_rejects_unknown_arch():
    import train as train_cli
    from manette_amd.exploration_policy import ExplorationPolicy
    from manette_amd.network import DeviceNetwork
    args = train_cli.get_arg_parser().parse_args(['-g', 'catcher', '--arch', 'BAYESIAN', '--keep_percentage', '0.8'])
    assert args.arch == 'BAYESIAN'
    args.random_seed = 3
    creator, _ = train_cli.get_network_and_environment_creator(args, ExplorationPolicy(args))
    conf = creator.__closure__[0].cell_contents
    assert conf['arch'] == 'BAYESIAN' and conf['keep_percentage'] == 0.8
    with pytest.raises(ValueError, match='BAYESIAN'):
        DeviceNetwork(dict(arch='BAYES', num_actions=6))
