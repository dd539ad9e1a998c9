"""numpy restatement of Catch, written from the rule's text in include/manette_hip.h ("Catch"), not from
the C++: plain Python integers for the game, numpy for the renders and the stack. Test infrastructure."""
import numpy as np

M64 = (1 << 64) - 1
SALT = 0xCA7C4BA11D0FF1E5
GRAY = {'ball': (255,), 'paddle': (160,)}
RGB = {'ball': (255, 64, 64), 'paddle': (64, 255, 64)}


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def tab_repetitions(max_repetition, nb_choices):
    """exploration_policy.py get_tab_repetitions."""
    res = [0] * nb_choices
    res[-1] = max_repetition
    for i in range(1, nb_choices - 1):
        res[i] = int(max_repetition / (nb_choices - 1)) * i
    return res


class Game(object):
    """One env. state() gives (paddle_x, ball_x, ball_y, ball_dx, misses, balls, ball_counter)."""

    def __init__(self, seed, global_env, depth=1, lives=3, max_balls=20):
        self.seed, self.env, self.depth = int(seed), int(global_env), depth
        self.lives, self.max_balls = lives, max_balls
        self.colors = GRAY if depth == 1 else RGB
        self.counter = 0
        self.px = self.bx = self.by = self.dx = self.misses = self.balls = 0

    def state(self):
        return (self.px, self.bx, self.by, self.dx, self.misses, self.balls, self.counter)

    def spawn(self):
        h = mix64(self.seed ^ mix64(((self.env << 40) & M64) ^ self.counter) ^ SALT)
        self.counter += 1
        self.bx = (h & 0xffffffff) % 81
        self.dx = ((h >> 32) % 3) - 1
        self.by = 0

    def render(self):
        """One render [84][84][depth] of the current positions; the ball is drawn over the paddle."""
        img = np.zeros((84, 84, self.depth), np.uint8)
        img[79:82, self.px:self.px + 12] = self.colors['paddle']
        img[self.by:self.by + 4, self.bx:self.bx + 4] = self.colors['ball']
        return img

    def next(self, a, render=True):
        """4 sub-frames; returns (frame or None, reward, over)."""
        reward, over, renders = 0, False, []
        for f in range(4):
            if not over:
                self.px = min(72, max(0, self.px + (-2 if a == 1 else 2 if a == 2 else 0)))
                self.by += 2
                self.bx += self.dx
                if self.bx < 0:
                    self.bx, self.dx = -self.bx, -self.dx
                elif self.bx > 80:
                    self.bx, self.dx = 160 - self.bx, -self.dx
                if self.by + 3 >= 79:
                    if self.bx < self.px + 12 and self.bx + 4 > self.px:
                        reward += 1
                    else:
                        reward -= 1
                        self.misses += 1
                    self.balls += 1
                    if self.misses >= self.lives or self.balls >= self.max_balls:
                        over = True
                    else:
                        self.spawn()
            if render and f >= 2:
                renders.append(self.render())
        return (np.maximum(renders[0], renders[1]) if render else None), reward, over

    def new_game(self, render=True):
        """Returns the four frames of the initial state (oldest first)."""
        self.px, self.misses, self.balls = 36, 0, 0
        self.spawn()
        return [self.next(0, render)[0] for _ in range(4)]

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


def stack(prev, frames, depth):
    """prev [84][84][4*depth] + the pushed frames -> the next stacked state (the last <= 4 frames; channel
    order [c_t0..c_t3 for each colour c])."""
    frames = frames[-4:]
    p = len(frames)
    st = prev.reshape(84, 84, depth, 4)
    out = np.empty_like(st)
    out[..., :4 - p] = st[..., p:]
    for j, f in enumerate(frames):
        out[..., 4 - p + j] = f
    return out.reshape(84, 84, 4 * depth)


def clamp_indices(a, r, R):
    return min(2, max(0, int(a))), min(R - 1, max(0, int(r)))


def hashed_actions(step, env, R):
    """The tests' deterministic (a, r) for (macro-step, env)."""
    h = mix64((step << 20) ^ env ^ 0x5151)
    return int(h % 3), int((h >> 20) % R)
