"""Crafted Bricks states (test infrastructure, shared by the CPU and the GPU tests): each case is a state
that forces one event of the rule within one next() under one action, with what the rule's text says must
come out of it. The state is caller-owned memory, so a test writes it directly. Defaults: lives 3,
max_nexts 500, serve_wait 4; every case is played with R = 1 (one next per macro-step)."""
from bricks_ref import FULL, M64


def st(bx, by, dx, dy, px=30, lives=3, nexts=10, wait=0, bricks=FULL, counter=5):
    return (px, bx, by, dx, dy, lives, nexts, wait, bricks & M64, bricks >> 64, 0, counter)


def parked(px, wait=0, lives=3):
    return st(px + 7, 77, 0, 0, px=px, wait=wait, lives=lives)


def _bit(k):
    return FULL & ~(1 << k)


# (name, state, action, expected reward of the first next, expected fields after it)
CASES = [
    # brick hits; 'bricks' is the 84-bit bitmap afterwards
    ('bit0', st(3, 14, -1, 2), 0, 1, dict(bricks=_bit(0), ball_y=10, ball_dy=-2, ball_x=1, ball_dx=1)),
    ('bit13', st(79, 14, 1, 2), 0, 1, dict(bricks=_bit(13), ball_dy=-2)),
    ('bit63_subframe3', st(41, 36, 1, -2, bricks=_bit(77)), 0, 1, dict(bricks=_bit(77) & _bit(63), ball_dy=2, ball_y=32)),
    ('bit64_subframe3', st(47, 36, 1, -2, bricks=_bit(78)), 0, 1, dict(bricks=_bit(78) & _bit(64), ball_dy=2, ball_y=32)),
    ('bit83', st(79, 36, 1, -2), 0, 1, dict(bricks=_bit(83), ball_dy=2)),
    ('bit76_subframe4', st(40, 40, -1, -2), 0, 1, dict(bricks=_bit(76), ball_x=36, ball_y=32, ball_dy=2)),
    ('last_brick_refills', st(40, 40, -1, -2, bricks=1 << 76), 0, 1, dict(bricks=FULL, ball_dy=2)),
    ('last_brick_refills_early', st(79, 36, 1, -2, bricks=1 << 83), 0, 1, dict(bricks=FULL)),
    # walls
    ('top_wall', st(40, 3, 2, -2), 0, 0, dict(ball_y=5, ball_dy=2, ball_x=48)),
    ('left_wall_x0', st(0, 50, -2, 2), 0, 0, dict(ball_x=8, ball_dx=2)),
    ('left_wall_x1', st(1, 50, -2, 2), 0, 0, dict(ball_x=7, ball_dx=2)),
    ('right_wall_x81', st(81, 50, 2, 2), 0, 0, dict(ball_x=75, ball_dx=-2)),
    ('right_wall_x82', st(82, 50, 2, 2), 0, 0, dict(ball_x=74, ball_dx=-2)),
] + [
    # paddle hits: off = ball_x + 1 - paddle_x at the test = o (paddle_x 30, the ball comes down with dx = +1)
    ('paddle_off%d' % o, st(28 + o, 76, 1, 2), 0, 0, dict(ball_dy=-2, ball_y=71, ball_dx=d, lives=3))
    for o, d in ((0, -2), (4, -2), (5, -1), (8, -1), (9, 1), (12, 1), (13, 2), (16, 2))
] + [
    ('miss_off-1', st(27, 76, 1, 2), 0, 0, dict(lives=2, ball_dy=0, ball_dx=0, ball_x=37, ball_y=77, wait=0)),
    ('miss_off17', st(45, 76, 1, 2, wait=3), 0, 0, dict(lives=2, ball_dy=0, ball_x=37, ball_y=77, wait=0)),
    ('miss_last_life', st(45, 76, 1, 2, lives=1), 0, 0, dict(lives=3, nexts=0, paddle_x=34, ball_dy=0, bricks=FULL)),
    # the paddle's clamps, the parked ball following it, the two ways to a serve
    ('clamp_left', parked(2), 3, 0, dict(paddle_x=0, ball_x=7, ball_y=77, ball_dy=0, wait=1)),
    ('clamp_right', parked(67), 2, 0, dict(paddle_x=68, ball_x=75, ball_dy=0, wait=1)),
    ('parked_follows', parked(34), 2, 0, dict(paddle_x=46, ball_x=53, ball_y=77, ball_dy=0, wait=1)),
    ('serve_by_fire', parked(34), 1, 0, dict(ball_y=44, ball_dy=2, serve_counter=6, wait=0)),
    ('serve_by_timeout', parked(34, wait=4), 0, 0, dict(ball_y=44, ball_dy=2, serve_counter=6, wait=4)),
    ('cap_ends_episode', st(40, 50, 1, 2, nexts=499), 0, 0, dict(nexts=0, lives=3, paddle_x=34, bricks=FULL)),
]
