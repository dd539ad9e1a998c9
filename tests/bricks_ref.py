"""numpy restatement of Bricks, written from the rule's text in include/manette_hip.h ("Bricks"), not from
the C++: plain Python integers for the game (the bitmap is one 84-bit integer), numpy for the renders and
the stack. Test infrastructure."""
import numpy as np

from catch_ref import M64, mix64, stack, tab_repetitions  # noqa: F401  (mix64 / stacking are Catch's)

SALT = 0xB41C5B0117A11E75
FULL = (1 << 84) - 1
DX = (-2, -1, 1, 2)
GRAY = {'ball': (255,), 'paddle': (160,), 'rows': [(90 + 20 * r,) for r in range(6)]}
RGB = {'ball': (255, 64, 64), 'paddle': (64, 255, 64),
       'rows': [(200, 72, 72), (198, 108, 58), (180, 122, 48), (162, 162, 42), (72, 160, 72), (66, 72, 200)]}
FIELDS = ('paddle_x', 'ball_x', 'ball_y', 'ball_dx', 'ball_dy', 'lives', 'nexts', 'wait', 'bricks_lo', 'bricks_hi',
          'reserved', 'serve_counter')


class Game(object):
    """One env. state() gives the fields of mt_bricks_state in their order."""

    def __init__(self, seed, global_env, depth=1, lives=3, max_nexts=500, serve_wait=4):
        self.seed, self.env, self.depth = int(seed), int(global_env), depth
        self.cfg_lives, self.max_nexts, self.serve_wait = lives, max_nexts, serve_wait
        self.colors = GRAY if depth == 1 else RGB
        self.counter = 0
        self.px = self.bx = self.by = self.dx = self.dy = self.lives = self.nexts = self.wait = 0
        self.bricks = 0

    def state(self):
        return (self.px, self.bx, self.by, self.dx, self.dy, self.lives, self.nexts, self.wait,
                self.bricks & M64, self.bricks >> 64, 0, self.counter)

    def load(self, t):
        """The inverse of state() (a crafted state)."""
        (self.px, self.bx, self.by, self.dx, self.dy, self.lives, self.nexts, self.wait, lo, hi, _, self.counter) = \
            [int(x) for x in t]
        self.bricks = lo | (hi << 64)

    def park(self):
        self.dy = self.dx = 0
        self.bx, self.by = self.px + 7, 77

    def render(self):
        """One render [84][84][depth]: the paddle, the bricks over it, the ball over both."""
        img = np.zeros((84, 84, self.depth), np.uint8)
        img[79:82, self.px:self.px + 16] = self.colors['paddle']
        for k in range(84):
            if (self.bricks >> k) & 1:
                r, c = divmod(k, 14)
                img[16 + 3 * r:19 + 3 * r, 6 * c:6 * c + 6] = self.colors['rows'][r]
        img[self.by:self.by + 2, self.bx:self.bx + 2] = self.colors['ball']
        return img

    def sub_frame(self, a):
        """Returns (reward, over)."""
        self.px = min(68, max(0, self.px + (3 if a == 2 else -3 if a == 3 else 0)))
        if self.dy == 0:
            self.bx = self.px + 7
            return 0, False
        reward = 0
        self.bx += self.dx
        if self.bx < 0:
            self.bx, self.dx = -self.bx, -self.dx
        elif self.bx > 82:
            self.bx, self.dx = 164 - self.bx, -self.dx
        self.by += self.dy
        if self.by < 0:
            self.by, self.dy = -self.by, -self.dy
        cy, cx = self.by + (self.dy > 0), self.bx + (self.dx > 0)
        if 16 <= cy < 34:
            k = 14 * ((cy - 16) // 3) + cx // 6
            if (self.bricks >> k) & 1:
                self.bricks &= ~(1 << k)
                reward += 1
                self.dy = -self.dy
                if self.bricks == 0:
                    self.bricks = FULL
        if self.dy > 0 and self.by + 1 >= 79:
            off = self.bx + 1 - self.px
            if 0 <= off <= 16:
                self.dy, self.by, self.dx = -2, 77, DX[min(3, 4 * off // 17)]
            else:
                self.lives -= 1
                if self.lives == 0:
                    return reward, True
                self.park()
                self.wait = 0
        return reward, False

    def next(self, a, render=True):
        """The serve decision and 4 sub-frames; returns (frame or None, reward, over)."""
        if self.dy == 0:
            if a == 1 or self.wait >= self.serve_wait:
                h = mix64(self.seed ^ mix64(((self.env << 40) & M64) ^ self.counter) ^ SALT)
                self.counter += 1
                self.bx, self.by, self.dy, self.dx = self.px + 7, 36, 2, DX[(h >> 32) & 3]
            else:
                self.wait += 1
        reward, over, renders = 0, False, []
        for f in range(4):
            if not over:
                rw, over = self.sub_frame(a)
                reward += rw
            if render and f >= 2:
                renders.append(self.render())
        self.nexts += 1
        over = over or self.nexts >= self.max_nexts
        return (np.maximum(renders[0], renders[1]) if render else None), reward, over

    def new_game(self, render=True):
        """Returns the four frames of the initial state: nothing is played."""
        self.px, self.lives, self.nexts, self.wait, self.bricks = 34, self.cfg_lives, 0, 0, FULL
        self.park()
        f = self.render() if render else None
        return [f, f, f, f]

    def macro_step(self, a, n, render=True):
        """n times next(a), stopping at an episode end (then a new game): (frames pushed since the last
        restart, summed reward, over)."""
        frames, total, over = [], 0, False
        for _ in range(n):
            f, rw, over = self.next(a, render)
            frames.append(f)
            total += rw
            if over:
                frames = self.new_game(render)
                break
        return frames, total, over


def clamp_indices(a, r, R):
    return min(3, max(0, int(a))), min(R - 1, max(0, int(r)))


def hashed_actions(step, env, R):
    """The tests' deterministic (a, r) for (macro-step, env): fire one time in 8, else noop / right / left."""
    h = mix64((step << 20) ^ env ^ 0xB51C)
    a = 1 if h % 8 == 0 else (0, 2, 3)[(h >> 8) % 3]
    return int(a), int((h >> 20) % R)
