"""The harness of tests/test_scratch_contract_gpu.py cannot hide a failure: for every workspace that
module poisons, the protected ranges mt_net_workspace_region reports are disjoint, inside the reported
size and word-aligned; scratch_util.poison changes every word outside them and only those, keeps the
argmax and mask bytes in range and leaves the counters and the dropout state alone; the arena's
buffers never overlap and keep their guards. mt_net_workspace_region and the size queries need no GPU
(tests/test_abi_refusals_cpu.py). CPU only."""
import ctypes as C

import numpy as np
import pytest
import torch

import scratch_util as su
import test_scratch_contract_gpu as gpu
from manette_amd import _lib


def _workspaces():
    """(arch, depth, layout, a, b) of every workspace the GPU module carves."""
    out = set()
    for arch, depth, _, _, _ in gpu.NETS_A:                       # (a), (b)
        for B in gpu.BATCHES:
            out.add((arch, depth, 2 if arch == 'LSTM' else 0, B, 0))
    for arch in ('NIPS', 'NATURE', 'PWYX'):                       # (c), (d)
        for E, T in gpu.ROLLOUTS:
            out.update({(arch, 1, 0, E, 0), (arch, 1, 0, T * E, 0)})
    for depth, E, T in ((1, 1, 1), (1, 3, 2), (3, 2, 2)):         # (e)
        out.add(('LSTM', depth, 1, E, T))
    for B in (1, 3, 9):                                           # (f)
        out.add(('BAYESIAN', 1, 0, B, 0))
    for arch, depth in (('NIPS', 1), ('NATURE', 1), ('PWYX', 1), ('PWYX', 3)):  # (g)
        for E in (1, 17):
            out.add((arch, depth, 0, E, 0))
    for B in (255, 256, 257, gpu.FUSED_CAP, gpu.FUSED_CAP + 1):   # the persistent trunk's boundary; the fused cap
        out.add(('NIPS', 1, 0, B, 0))
    return sorted(out)


WORKSPACES = _workspaces()
IDS = ['%s-%d-L%d-%d-%d' % w for w in WORKSPACES]


@pytest.fixture(scope='module')
def handles():
    lib, made = _lib.hip(), {}
    for arch, depth in sorted({w[:2] for w in WORKSPACES}):
        cfg = _lib.mt_net_config(_lib.MT_ARCH[arch], depth, 6, 3, 0, 0.1, 1.0, 0.5)
        h = C.c_void_p()
        _lib.check(lib.mt_net_create(C.byref(cfg), C.byref(h)))
        made[(arch, depth)] = h
    yield made
    for h in made.values():
        lib.mt_net_destroy(h)


@pytest.mark.parametrize('arch,depth,layout,a,b', WORKSPACES, ids=IDS)
def test_protected_regions_geometry(handles, arch, depth, layout, a, b):
    h = handles[(arch, depth)]
    total = su.workspace_bytes(h, layout, a, b)
    regions = su.protected_regions(h, layout, a, b)
    assert total % 4 == 0
    end = 0
    for kind, off, n in regions:  # (sorted by offset)
        assert kind in (su.KIND_ARGMAX, su.KIND_COUNTERS, su.KIND_MASK, su.KIND_STATE)
        assert off % 4 == 0 and n % 4 == 0 and n > 0, (kind, off, n)
        assert off >= end, ('overlap', kind, off, end)
        end = off + n
    assert end <= total
    kinds = [r[0] for r in regions]
    pooled = {'PWYX': 3, 'LSTM': 3}.get(arch, 0)  # 2x2 max pools behind conv1..conv3 (networks.py)
    assert kinds.count(su.KIND_ARGMAX) == pooled
    assert (su.KIND_STATE in kinds) == (su.KIND_MASK in kinds) == (arch == 'BAYESIAN')
    assert (su.KIND_COUNTERS in kinds) == (layout == 0 and arch in ('NATURE', 'PWYX') and (arch, depth) != ('NATURE', 3))


@pytest.mark.parametrize('pattern', su.PATTERNS)
@pytest.mark.parametrize('arch,depth,layout,a,b', WORKSPACES, ids=IDS)
def test_poison_touches_every_scratch_word_and_only_those(handles, arch, depth, layout, a, b, pattern):
    h = handles[(arch, depth)]
    total = su.workspace_bytes(h, layout, a, b)
    regions = su.protected_regions(h, layout, a, b)
    ws = np.zeros(total, np.uint8)
    for kind, off, n in regions:
        ws[off:off + n] = 0xFF if kind in (su.KIND_ARGMAX, su.KIND_MASK) else 0x11
    su.poison(ws, regions, pattern, np.random.RandomState(a))
    scratch = np.ones(total // 4, bool)
    for kind, off, n in regions:
        scratch[off // 4:(off + n) // 4] = False
        part = ws[off:off + n]
        if kind == su.KIND_ARGMAX:
            assert part.max() <= 3 and len(np.unique(part)) == 4
        elif kind == su.KIND_MASK:
            assert part.max() <= 1 and part.any() and not part.all()
        else:  # the counters and the dropout state: exactly as they were
            assert (part == 0x11).all(), kind
    words = ws.view(np.uint32)[scratch]
    if pattern == 'nan':
        assert (words == su.NAN_WORD).all()
    else:
        mag = np.abs(words.view(np.float32))
        assert np.isfinite(mag).all() and mag.min() >= su.STALE_LO and mag.max() <= su.STALE_HI
        assert (words.view(np.int32) < 0).any() and (words.view(np.int32) > 0).any()  # both signs


def test_nan_word_is_a_quiet_nan():
    x = np.array([su.NAN_WORD], np.uint32).view(np.float32)[0]
    assert np.isnan(x) and (su.NAN_WORD >> 22) & 1


def test_grad_poison_keeps_the_padding_zero():
    class Net(object):  # two variables with a gap between and after them
        nparams = 192
        vars = [('a', (5, 7), 0, 0.1), ('b', (3,), 64, 0.1)]
    for pattern in su.PATTERNS:
        net = Net()
        net.grad = torch.zeros(net.nparams)
        su.grad_poison(net, pattern, 3)
        g, m = net.grad.numpy(), su.var_mask(net)
        assert m.sum() == 38 and not g[~m].view(np.uint32).any()
        assert (g[m].view(np.uint32) == su.NAN_WORD).all() if pattern == 'nan' else (np.abs(g[m]) >= su.STALE_LO).all()


@pytest.mark.parametrize('sizes', [[1], [4, 1, 65536, 3], [255, 256, 257], [100000, 7, 1 << 20]])
def test_arena_layout_keeps_alignment_and_guards(sizes):
    slots, total = su.arena_layout({i: n for i, n in enumerate(sizes)})
    at = 0
    for i, n in enumerate(sizes):
        off, m = slots[i]
        assert m == n and off % su.ALIGN == 0 and off - at >= su.GUARD
        at = off + n
    assert total - at >= su.GUARD


def test_arena_check_sees_a_byte_in_any_guard():
    arena = su.Arena({'a': 100, 'b': 4096}, device='cpu')
    assert arena.buf('a').numel() == 100 and arena.buf('b', torch.float32).numel() == 1024
    arena.buf('a').fill_(7)
    arena.buf('b').fill_(su.SENTINEL ^ 0xFF)
    arena.check()
    gaps = arena.gaps()
    assert len(gaps) == 3 and all(hi - lo >= su.GUARD for lo, hi in gaps)
    for lo, hi in gaps:
        for at in (lo, hi - 1):  # the bytes right behind and right before a buffer, and the arena's ends
            arena.mem[at] = 0
            with pytest.raises(AssertionError):
                arena.check()
            arena.mem[at] = su.SENTINEL
    arena.check()
