"""--bayes_native without a GPU: the rollout flag and the fused update's prototype in the ctypes
bindings and the header, the CLI flag, and the arch validation (raised before any device allocation)."""
import ctypes as C
import os
import re
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli():
    sys.path.insert(0, ROOT)
    import train
    return train


def test_lib_exposes_flag_and_prototype():
    from manette_amd import _lib
    assert _lib.MT_ROLLOUT_DROPOUT == 64
    flags = [getattr(_lib, n) for n in dir(_lib) if n.startswith('MT_ROLLOUT_')]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)  # distinct single bits
    res, args = _lib._HIP_SIGS['mt_dropout_returns_loss_backward']
    assert res is C.c_int and len(args) == 24
    assert args[3] is C.c_int and args[4] is C.c_int and args[6] is C.c_size_t
    assert args[13] is C.c_double and args[19] is C.c_float
    assert all(a is C.c_void_p for i, a in enumerate(args) if i not in (3, 4, 6, 13, 19))
    with open(os.path.join(ROOT, 'include', 'manette_hip.h')) as f:
        text = f.read()
    assert re.search(r'#define\s+MT_ROLLOUT_DROPOUT\s+64\b', text)
    proto = re.search(r'int mt_dropout_returns_loss_backward\(([^;]*)\);', text)
    assert proto and len(proto.group(1).split(',')) == 24
    if os.path.exists(_lib.HIP_LIB):  # (a built tree: the symbol resolves)
        assert _lib.hip().mt_dropout_returns_loss_backward is not None


def test_parser_accepts_bayes_native():
    p = _cli().get_arg_parser()
    assert p.parse_args([]).bayes_native is False
    a = p.parse_args(['--arch', 'BAYESIAN', '--bayes_native'])
    assert a.bayes_native is True and a.arch == 'BAYESIAN'
    _cli().validate_args(a)


def test_flag_is_saved_in_args_json(tmp_path):
    import json
    from manette_amd import logger_utils
    a = _cli().get_arg_parser().parse_args(['--arch', 'BAYESIAN', '--bayes_native'])
    logger_utils.save_args(a, str(tmp_path) + '/')
    with open(os.path.join(str(tmp_path), 'args.json')) as f:
        assert json.load(f)['bayes_native'] is True


@pytest.mark.parametrize('arch', ['NIPS', 'NATURE', 'PWYX', 'LSTM'])
def test_flag_with_another_arch_raises(arch):
    cli = _cli()
    a = cli.get_arg_parser().parse_args(['--arch', arch, '--bayes_native'])
    with pytest.raises(ValueError, match='bayes_native'):
        cli.validate_args(a)
    from manette_amd.paac import PAACLearner, check_arch_flags
    with pytest.raises(ValueError, match='bayes_native'):
        check_arch_flags(a)

    def never(*_a, **_k):
        raise AssertionError('a creator ran before the flag check')

    # the learner refuses before it builds a network or an environment
    with pytest.raises(ValueError, match='bayes_native'):
        PAACLearner(never, types.SimpleNamespace(create_environment=never), types.SimpleNamespace(tab_rep=[1]), a)
    check_arch_flags(cli.get_arg_parser().parse_args(['--arch', arch]))
