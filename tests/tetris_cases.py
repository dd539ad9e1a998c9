"""Crafted Tetris states for single acts: (name, state, action). tests/golden/make_golden_tetris.py sets each
into the reference's TetrisApp and records what its act() makes of it (tests/golden/tetris_rule.npz, case_*);
the tests replay them on mt_tetris_step_host and, as one batch, on the kernel. Data only."""
SEED = 0x7E7215
ENV = 3


def board(rows=None):
    """22 rows of 10 cells from {row: 'ten digits'}."""
    b = [[0] * 10 for _ in range(22)]
    for y, cells in (rows or {}).items():
        assert len(cells) == 10
        b[y] = [int(c) for c in cells]
    return b


def st(rows, piece, rot, x, y, next_piece=1, level=1, lines=0, speed=5, speed_counter=1, piece_counter=9):
    return dict(board=board(rows), piece=piece, rot=rot, x=x, y=y, next_piece=next_piece, level=level, lines=lines,
                speed=speed, speed_counter=speed_counter, nexts=10, piece_counter=piece_counter)


GAP2 = '1111111100'  # open at columns 8, 9 (the O piece at x = 8)
GAP1 = '2222222220'  # open at column 9 (the upright I piece at x = 9)

CASES = [
    ('clear_1', st({21: GAP2}, 7, 0, 8, 20), 3),
    ('clear_2', st({20: GAP2, 21: GAP2}, 7, 0, 8, 20, level=3, lines=13), 3),
    ('clear_3', st({18: '3000000000', 19: GAP1, 20: GAP1, 21: GAP1}, 6, 1, 9, 18), 3),
    ('clear_4', st({18: GAP1, 19: GAP1, 20: GAP1, 21: GAP1}, 6, 1, 9, 18, level=2, lines=7), 3),
    ('clear_levels_up', st({21: GAP2}, 7, 0, 8, 20, lines=5), 3),
    ('clear_4_levels_up_once', st({18: GAP1, 19: GAP1, 20: GAP1, 21: GAP1}, 6, 1, 9, 18, lines=10), 3),
    ('level_up_speed_already_1', st({21: GAP2}, 7, 0, 8, 20, lines=5, speed=1), 3),
    ('over_on_spawn_with_full_row', st({0: '0001111000', 1: '0001111000', 21: GAP2}, 7, 0, 8, 20, next_piece=6), 3),
    ('drop_locks_then_gravity', st({21: '0000000011'}, 7, 0, 8, 19, next_piece=4, speed_counter=5), 3),
    ('drop_does_not_lock', st({}, 2, 1, 4, 7), 3),
    ('rotate', st({}, 1, 0, 4, 7), 4),
    ('rotate_refused_right_wall', st({}, 6, 1, 9, 5), 4),
    ('rotate_refused_bottom', st({}, 6, 0, 3, 21), 4),
    ('rotate_refused_by_stack', st({10: '0000001000'}, 6, 1, 4, 10), 4),
    ('move_left', st({}, 5, 2, 4, 3), 1),
    ('move_right', st({}, 5, 3, 4, 3), 2),
    ('move_left_clamped', st({}, 1, 0, 0, 6), 1),
    ('move_right_clamped', st({}, 1, 0, 7, 6), 2),
    ('move_left_refused', st({10: '0010000000'}, 1, 0, 3, 10), 1),
    ('move_right_refused', st({11: '0000000500'}, 3, 0, 4, 10), 2),
    ('gravity_only_lock', st({}, 7, 0, 0, 20, speed_counter=10), 0),
    ('gravity_only_lock_clears', st({21: GAP2}, 7, 0, 8, 20, speed_counter=0, level=2, lines=6), 0),
    ('noop_without_gravity', st({21: GAP2}, 7, 0, 8, 20), 0),
]
