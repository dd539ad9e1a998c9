"""Helpers of the scratch-contract tests (not a test module; importing it needs no GPU).

The contract (include/manette_hip.h): of everything a net entry point is handed, only the hand-off
counters (mt_net_workspace_region kind 4), the BAYESIAN dropout state (kind 7) and the once-zeroed
alignment padding of the gradient persist between calls. Every other workspace word, every output and
every variable's gradient is scratch: a call sequence gives the same bits whatever they held before,
and writes nothing outside the buffers it was handed at the sizes the size queries report.

- protected_regions: the byte ranges of a workspace that are not fp32 scratch, read from the library;
- poison / grad_poison / fill: put a workspace, the gradient or an output into the `nan` or `stale` state;
- Arena: one allocation of sentinel bytes the test carves every written buffer out of, with guards.
"""
import ctypes as C

import numpy as np
import torch

from manette_amd import _lib

KIND_ARGMAX, KIND_COUNTERS, KIND_MASK, KIND_STATE = 1, 4, 5, 7
MAX_CONV_LAYERS = 4            # WsLayout keeps four conv layers at the most
NAN_WORD = 0x7FC00000          # the quiet NaN
STALE_LO, STALE_HI = 1e3, 1e6  # magnitudes another call would have left, large enough to wreck a sum
PATTERNS = ('nan', 'stale')

GUARD = 64 * 1024
ALIGN = 256
SENTINEL = 0xA5


def _handle(net):
    return getattr(net, '_h', net)


def workspace_bytes(net, layout, a, b=0):
    """mt_net_workspace_bytes (layout 0: a rows; 2: an LSTM forward of a windows) or
    mt_lstm_frames_workspace_bytes (layout 1: E = a, T = b)."""
    n = C.c_size_t()
    if int(layout) == 1:
        _lib.check(_lib.hip().mt_lstm_frames_workspace_bytes(_handle(net), int(a), int(b), C.byref(n)))
    else:
        _lib.check(_lib.hip().mt_net_workspace_bytes(_handle(net), int(a), C.byref(n)))
    return n.value


def protected_regions(net, layout, a, b=0):
    """[(kind, byte offset, bytes)] of every non-empty range of the workspace that is not fp32 scratch,
    from mt_net_workspace_region: kind 1 = a pooled layer's max-pool argmax bytes (one range per pooled
    layer, any layout), and in the layout-0 workspace kind 4 = the hand-off counters, kind 5 = the
    BAYESIAN mask bytes, kind 7 = the dropout state. Everything else in ws_layout, lstm_ws_layout and
    the frame-store layout is fp32. A (kind, layer) the arch does not have is refused by the library and
    skipped here. net: a DeviceNetwork or an mt_net handle."""
    lib, h = _lib.hip(), _handle(net)
    out = []

    def ask(kind, layer):
        off, n = C.c_size_t(), C.c_size_t()
        rc = lib.mt_net_workspace_region(h, int(layout), int(a), int(b), kind, layer, C.byref(off), C.byref(n))
        if rc == 0 and n.value:
            out.append((kind, off.value, n.value))

    for layer in range(MAX_CONV_LAYERS):
        ask(KIND_ARGMAX, layer)
    if int(layout) == 0:
        for kind in (KIND_COUNTERS, KIND_MASK, KIND_STATE):
            ask(kind, 0)
    return sorted(out, key=lambda r: r[1])


def _as_tensor(buf):
    return torch.from_numpy(buf) if isinstance(buf, np.ndarray) else buf


def _generator(t, rng):
    """A torch generator on t's device seeded from rng (an int, or a numpy RandomState that is advanced)."""
    seed = int(rng.randint(0, 2 ** 31 - 1)) if hasattr(rng, 'randint') else int(rng)
    return torch.Generator(device=t.device).manual_seed(seed)


def _stale_words(n, t, gen):
    mag = torch.rand(n, generator=gen, device=t.device, dtype=torch.float32) * (STALE_HI - STALE_LO) + STALE_LO
    mag = mag.clamp_(STALE_LO, STALE_HI)
    sign = torch.randint(0, 2, (n,), generator=gen, device=t.device, dtype=torch.int32).float() * 2 - 1
    return mag * sign


def fill(t, pattern, rng):
    """A float32 (or int32-viewed) buffer into the pattern: 'zero', 'nan' (every word the quiet NaN) or
    'stale' (random finite floats, magnitude in [1e3, 1e6], random sign)."""
    t = _as_tensor(t)
    flat = t.reshape(-1).view(torch.int32)
    if pattern == 'zero':
        flat.zero_()
    elif pattern == 'nan':
        flat.fill_(NAN_WORD)
    elif pattern == 'stale':
        flat.view(torch.float32).copy_(_stale_words(flat.numel(), flat, _generator(flat, rng)))
    else:
        raise ValueError(pattern)
    return t


def poison(ws, regions, pattern, rng):
    """Every 32-bit word of the uint8 workspace `ws` (a numpy array or a torch tensor, host or device)
    outside the protected `regions` becomes the pattern. Kind-1 bytes become random window positions
    0..3 and kind-5 bytes random 0 / 1, so a stale read of one gives a wrong number and never an address
    out of range; kinds 4 and 7 (the counters, which must stay zero, and the dropout state, which the
    test seeds) are left exactly as they were."""
    assert pattern in PATTERNS, pattern
    t = _as_tensor(ws)
    assert t.dtype == torch.uint8 and t.dim() == 1 and t.numel() % 4 == 0
    gen = _generator(t, rng)
    keep = [(off, t[off:off + n].clone()) for kind, off, n in regions if kind in (KIND_COUNTERS, KIND_STATE)]
    fill(t.view(torch.int32), pattern, int(torch.randint(0, 2 ** 31 - 1, (1,), generator=gen, device=t.device)))
    for kind, off, n in regions:
        if kind in (KIND_ARGMAX, KIND_MASK):
            hi = 4 if kind == KIND_ARGMAX else 2
            t[off:off + n] = torch.randint(0, hi, (n,), generator=gen, device=t.device, dtype=torch.uint8)
    for off, saved in keep:
        t[off:off + saved.numel()] = saved
    return ws


def var_mask(net):
    """Boolean [nparams]: True inside a variable, False in the alignment padding of the flat layout."""
    m = np.zeros(net.nparams, bool)
    for _, shape, off, _ in net.vars:
        m[off:off + int(np.prod(shape))] = True
    return m


def grad_poison(net, pattern, rng):
    """net.grad's variables into the pattern; the alignment padding stays zero, as the contract says
    (mt_loss_backward never touches it and the clip's norm sums the whole buffer)."""
    fill(net.grad, pattern, rng)
    pad = torch.from_numpy(~var_mask(net)).to(net.grad.device)
    net.grad[pad] = 0.0


def arena_layout(sizes, guard=GUARD, align=ALIGN):
    """{name: (offset, bytes)} and the total of an arena holding `sizes` ({name: bytes}, in order): every
    offset a multiple of `align`, at least `guard` bytes before the first buffer, between two buffers
    and after the last."""
    up = lambda x: -(-x // align) * align
    off, out = up(guard), {}
    for name, n in sizes.items():
        assert n > 0, (name, n)
        out[name] = (off, int(n))
        off = up(off + int(n) + guard)
    return out, off


class Arena(object):
    """One allocation filled with the sentinel byte; buf(name) is the uint8 view of a carved buffer
    (exactly its size), check() asserts that every byte outside the carved buffers still holds the
    sentinel: a write past the end of — or before — anything the call was handed lands in a guard."""

    def __init__(self, sizes, device='cuda'):
        self.slots, self.total = arena_layout(sizes)
        raw = torch.full((self.total + ALIGN,), SENTINEL, dtype=torch.uint8, device=device)
        shift = -raw.data_ptr() % ALIGN  # (a host allocation is 64-byte aligned only)
        self.mem = raw[shift:shift + self.total]
        assert self.mem.data_ptr() % ALIGN == 0

    def buf(self, name, dtype=torch.uint8):
        off, n = self.slots[name]
        return self.mem[off:off + n].view(dtype)

    def gaps(self):
        """The guard ranges [(begin, end)]: everything outside the carved buffers."""
        out, at = [], 0
        for off, n in sorted(self.slots.values()):
            out.append((at, off))
            at = off + n
        out.append((at, self.total))
        return out

    def check(self):
        bad = []
        for lo, hi in self.gaps():
            hit = torch.nonzero(self.mem[lo:hi] != SENTINEL)
            if hit.numel():
                near = [k for k, (off, n) in self.slots.items() if off + n == lo or off == hi]
                bad.append((near, lo + int(hit[0]), int(hit.numel())))
        assert not bad, ('bytes written outside the declared buffers (buffers beside the guard, first byte, count)',
                         bad)
