"""Python restatement of Tetris' draws, shapes and render, written from the rule's text in include/manette_hip.h
("Tetris"), not from the C++; a scripted placement policy; and the glue between the recorded fields of
tests/golden/tetris_rule.npz (taken from the reference's own TetrisApp by tests/golden/make_golden_tetris.py)
and mt_tetris_state. Test infrastructure."""
import numpy as np

from catch_ref import M64, mix64, stack, tab_repetitions  # noqa: F401  (mix64 / stacking are Catch's)

SALT = 0x7E7215B10C5D20F7
WAIT_SALT = 0x57A27F0A17C0FFEE
COLS, ROWS = 10, 22
SHAPES = [
    [[1, 1, 1], [0, 1, 0]],
    [[0, 2, 2], [2, 2, 0]],
    [[3, 3, 0], [0, 3, 3]],
    [[4, 0, 0], [4, 4, 4]],
    [[0, 0, 5], [5, 5, 5]],
    [[6, 6, 6, 6]],
    [[7, 7], [7, 7]],
]
RGB = [(0, 0, 0), (255, 85, 85), (100, 200, 115), (120, 108, 245), (255, 140, 50), (50, 120, 52), (146, 202, 73),
       (150, 161, 218), (35, 35, 35)]
GRAY = [0, 136, 160, 127, 164, 91, 171, 190, 35]
LINE_SCORES = (0, 40, 100, 300, 1200)
FIELDS = ('piece', 'rot', 'x', 'y', 'next_piece', 'level', 'lines', 'speed', 'speed_counter', 'nexts')


def draw(seed, genv, counter, salt=SALT):
    """The hash of draw `counter` of env genv."""
    return mix64(seed ^ mix64(((genv << 40) & M64) ^ counter) ^ salt)


def piece_draw(seed, genv, counter):
    """Shape index 0..6 (id - 1)."""
    return draw(seed, genv, counter) % 7


def start_wait(seed, genv, counter, max_start_wait):
    return draw(seed, genv, counter, WAIT_SALT) % (max_start_wait + 1)


def rotate(m):
    """new[i][j] = old[j][W-1-i]."""
    h, w = len(m), len(m[0])
    return [[m[j][w - 1 - i] for j in range(h)] for i in range(w)]


def matrix(piece, rot):
    m = SHAPES[piece - 1]
    for _ in range(rot % 4):
        m = rotate(m)
    return m


def rot_of(piece, cells):
    """The smallest rot whose matrix is `cells` (a list of rows)."""
    for r in range(4):
        if matrix(piece, r) == [list(map(int, row)) for row in cells]:
            return r
    raise ValueError('not a rotation of shape %d: %r' % (piece, cells))


def board_words(board):
    """[22][10] colour ids -> 22 words, cell x at bits 3x..3x+2."""
    return [sum(int(c) << (3 * x) for x, c in enumerate(row)) for row in board]


def words_board(words):
    return np.asarray([[(int(w) >> (3 * x)) & 7 for x in range(COLS)] for w in words], np.uint8)


def fill_state(st, board, piece, rot, x, y, next_piece, level, lines, speed, speed_counter, nexts, piece_counter):
    """Write the fields into a ctypes mt_tetris_state."""
    for i, w in enumerate(board_words(board)):
        st.board[i] = w
    for n, v in zip(FIELDS, (piece, rot, x, y, next_piece, level, lines, speed, speed_counter, nexts)):
        setattr(st, n, int(v))
    st.piece_counter = int(piece_counter)
    return st


def state_tuple(board, piece, rot, x, y, next_piece, level, lines, speed, speed_counter, nexts, piece_counter):
    """The same as one record of tetris.STATE_DTYPE."""
    return (board_words(board), piece, rot, x, y, next_piece, level, lines, speed, speed_counter, nexts, piece_counter)


# ---- render ----------------------------------------------------------------------------------------
def cell_ids(board, piece, rot, x, y, next_piece):
    """[22][16] colour ids of the screen's cells, drawn in the rule's order."""
    ids = np.zeros((ROWS, 16), np.uint8)
    for cy in range(ROWS):
        for cx in range(COLS):
            if cx % 2 == cy % 2:
                ids[cy, cx] = 8
            if board[cy][cx]:
                ids[cy, cx] = board[cy][cx]
    for m, (ox, oy), c in ((matrix(piece, rot), (x, y), piece), (matrix(next_piece, 0), (11, 2), next_piece)):
        for r, row in enumerate(m):
            for k, v in enumerate(row):
                if v and oy + r < ROWS and ox + k < 16:
                    ids[oy + r, ox + k] = c
    return ids


def sample_rows():
    return [(((2 * i + 1) * 33) // 14) // 18 for i in range(84)]


def sample_cols():
    return [(((2 * j + 1) * 12) // 7) // 18 for j in range(84)]


def render(board, piece, rot, x, y, next_piece, depth):
    """One frame [84][84][depth]."""
    ids = cell_ids(board, piece, rot, x, y, next_piece)
    pix = ids[np.asarray(sample_rows())][:, np.asarray(sample_cols())]
    table = np.asarray(GRAY, np.uint8)[:, None] if depth == 1 else np.asarray(RGB, np.uint8)
    return table[pix]


def render_state(rec, depth):
    """A frame from one record of tetris.STATE_DTYPE (or a ctypes state)."""
    g = (lambda n: rec[n]) if isinstance(rec, np.void) else (lambda n: getattr(rec, n))
    return render(words_board(list(g('board'))), int(g('piece')), int(g('rot')), int(g('x')), int(g('y')),
                  int(g('next_piece')), depth)


def hashed_actions(step, env, R):
    """The tests' deterministic (a, r) for (macro-step, env)."""
    h = mix64((step << 20) ^ env ^ 0x7E75)
    return int(h % 5), int((h >> 20) % R)


# ---- a scripted placement policy -------------------------------------------------------------------
def _collides(occ, m, x, y):
    """occ: 22 ints, bit x set where the cell is occupied."""
    for r, row in enumerate(m):
        for k, v in enumerate(row):
            if v:
                if x + k >= COLS or y + r >= ROWS or (occ[y + r] >> (x + k)) & 1:
                    return True
    return False


def _evaluate(occ, m, x, y):
    rows = list(occ)
    for r, row in enumerate(m):
        for k, v in enumerate(row):
            if v:
                rows[y + r] |= 1 << (x + k)
    full = (1 << COLS) - 1
    kept = [w for w in rows if w != full]
    cleared = ROWS - len(kept)
    rows = [0] * cleared + kept
    heights, holes = [], 0
    for cx in range(COLS):
        h = 0
        for cy in range(ROWS):
            if (rows[cy] >> cx) & 1:
                if h == 0:
                    h = ROWS - cy
            elif h:
                holes += 1
        heights.append(h)
    bump = sum(abs(heights[i] - heights[i + 1]) for i in range(COLS - 1))
    return -0.51 * sum(heights) + 0.76 * cleared - 0.36 * holes - 0.18 * bump


class PlacementPolicy(object):
    """Chooses, once per piece (key: anything that changes when a new piece spawns), the rotation and column
    whose straight drop scores best under a height / holes / bumpiness / rows heuristic, then steers there:
    rotate, move, and drop once in place."""

    def __init__(self):
        self.key, self.target = None, None

    def action(self, key, board, piece, rot, x, y):
        occ = [sum(1 << cx for cx in range(COLS) if board[cy][cx]) for cy in range(ROWS)]
        if key != self.key:
            best = None
            for dr in range(4):
                m = matrix(piece, rot + dr)
                for tx in range(COLS - len(m[0]) + 1):
                    if _collides(occ, m, tx, y):
                        continue
                    ty = y
                    while not _collides(occ, m, tx, ty + 1):
                        ty += 1
                    sc = _evaluate(occ, m, tx, ty)
                    if best is None or sc > best[0]:
                        best = (sc, (rot + dr) % 4, tx)
            self.key, self.target = key, (best[1:] if best else (rot % 4, x))
        trot, tx = self.target
        if rot % 4 != trot:
            if _collides(occ, matrix(piece, rot + 1), x, y):  # refused here: step away from the right wall
                return 1 if x > 0 else 3
            return 4
        if tx < x:
            return 1
        if tx > x:
            return 2
        return 3
