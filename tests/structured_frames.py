"""Atari-like frames for the parity tests (not a test module).

The other parity tests feed the kernels uniform noise, where no two receptive fields are alike. A
real frame is a constant background with a few sprites, stacked four times with little motion: most
2x2 pool windows of the PWYX / LSTM trunk then see four byte-identical receptive fields, tie exactly,
and the backward's "first maximum" rule decides where the gradient goes.
"""
import numpy as np

from oracle import nets

# what tests/test_structured_frames_{cpu,gpu}.py run on: the CPU test proves for exactly these frames
# and initial weights that the GPU tests' tie checks are not vacuous
B = 6
SEED = 5


def frames(seed, B, depth):
    """uint8 [B, 84, 84, 4 * depth], deterministic: per frame one background colour per colour plane
    and up to three rectangles (2-16 high, 1-8 wide, one colour per plane) that move by 0-2 pixels in
    y and x per stacked time step; channel c = 4 * plane + t ([R_t0..R_t3, G_t0.., B_t0..]); row 0 is
    all 0 and row 1 all 255 (the extremes of the input scale, in every frame)."""
    rs = np.random.RandomState(seed)
    x = np.zeros((B, 84, 84, 4 * depth), np.uint8)
    for b in range(B):
        x[b] = np.repeat(rs.randint(0, 256, size=depth), 4).astype(np.uint8)
        for _ in range(rs.randint(0, 4) if b else 3):  # (frame 0 always carries three)
            h, w = rs.randint(2, 17), rs.randint(1, 9)
            y0, x0 = rs.randint(2, 84 - h), rs.randint(0, 84 - w)
            vy, vx = rs.randint(-2, 3), rs.randint(-2, 3)
            col = rs.randint(0, 256, size=depth)
            for t in range(4):
                ya, xa = np.clip(y0 + vy * t, 0, 84 - h), np.clip(x0 + vx * t, 0, 84 - w)
                x[b, ya:ya + h, xa:xa + w, t::4] = col
        x[b, 0] = 0
        x[b, 1] = 255
    return x


def identical_windows(x, k):
    """x [B, H, W, C] (any dtype): the input of a stride-1 SAME k x k conv followed by the 2x2 / 2 pool.
    Returns bool [B, H // 2, W // 2]: the pool windows whose four zero-padded receptive fields are
    element-wise identical — whatever the weights, such a window's four conv outputs are the same
    sums of the same numbers."""
    x = np.asarray(x)
    Bn, H, W, _ = x.shape
    cols, _ = nets.im2col(x, k, 1, 'SAME')
    OH, OW = H // 2, W // 2
    f = cols.reshape(Bn, H, W, -1)[:, :2 * OH, :2 * OW].reshape(Bn, OH, 2, OW, 2, -1)
    first = f[:, :, :1, :, :1]
    return (f == first).all(axis=(2, 4, 5))
