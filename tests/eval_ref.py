"""A numpy restatement of the three device-evaluation rules (include/manette_hip.h, "Device evaluation"),
written from the rule text and independent of the C code (not a test module; needs no GPU).

EvalRef holds the state as numpy arrays; reset / step / summarize follow the rules, summarize in the
rule's order (256 lanes, ascending entries per lane, then the halving tree), so its doubles are the
kernel's bit for bit.
"""
import numpy as np

LANES = 256


class EvalRef(object):
    def __init__(self, N, K):
        self.N, self.K = int(N), int(K)
        self.ret_acc = np.full(N, 7.0, np.float32)  # (garbage until reset)
        self.len_acc = np.full(N, 7, np.int64)
        self.done = np.full(N, 7, np.int32)
        self.returns = np.full((N, K), 7.0, np.float32)
        self.lengths = np.full((N, K), 7, np.int64)
        self.remaining, self.steps = -1, -1

    def reset(self):
        for a in (self.ret_acc, self.len_acc, self.done, self.returns, self.lengths):
            a[...] = 0
        self.remaining, self.steps = self.N * self.K, 0

    def step(self, r_idx, reward, over, tab_rep):
        R = len(tab_rep)
        live = self.done < self.K
        r = np.clip(np.asarray(r_idx, np.int64), 0, R - 1)
        nexts = np.clip(np.asarray(tab_rep, np.int64)[r], 0, 255) + 1
        ret = (self.ret_acc + np.asarray(reward, np.float32)).astype(np.float32)
        ln = self.len_acc + nexts
        ended = live & (np.asarray(over, np.float32) != 0)
        e = np.nonzero(ended)[0]
        self.returns[e, self.done[e]] = ret[e]
        self.lengths[e, self.done[e]] = ln[e]
        self.done[e] += 1
        ret[e] = 0
        ln[e] = 0
        self.ret_acc[live] = ret[live]
        self.len_acc[live] = ln[live]
        self.remaining = int((self.K - self.done.astype(np.int64)).sum())
        self.steps += 1

    def summarize(self):
        """dict of the summary's fields."""
        N, K = self.N, self.K
        NK = N * K
        rows = -(-NK // LANES)
        pad = rows * LANES - NK
        counted = (np.arange(K)[None, :] < self.done[:, None]).reshape(-1)
        counted = np.concatenate([counted, np.zeros(pad, bool)]).reshape(rows, LANES)
        ret = np.concatenate([self.returns.reshape(-1), np.zeros(pad, np.float32)]).reshape(rows, LANES)
        ln = np.concatenate([self.lengths.reshape(-1), np.zeros(pad, np.int64)]).reshape(rows, LANES)
        n = np.zeros(LANES, np.int64)
        lsum = np.zeros(LANES, np.int64)
        s = np.zeros(LANES, np.float64)
        ss = np.zeros(LANES, np.float64)
        mn = np.zeros(LANES, np.float32)
        mx = np.zeros(LANES, np.float32)
        for q in range(rows):  # lane j meets entry q * 256 + j: ascending per lane
            c = counted[q]
            x = ret[q].astype(np.float64)
            first = c & (n == 0)
            mn = np.where(first, ret[q], np.where(c & (ret[q] < mn), ret[q], mn))
            mx = np.where(first, ret[q], np.where(c & (ret[q] > mx), ret[q], mx))
            n = n + c
            lsum = lsum + np.where(c, ln[q], 0)
            s = np.where(c, s + x, s)
            ss = np.where(c, ss + x * x, ss)
        h = LANES // 2
        while h >= 1:  # part[j] (+)= part[j + h]; an empty side gives nothing to min / max
            a, b = slice(0, h), slice(h, 2 * h)
            has_a, has_b = n[a] != 0, n[b] != 0
            mn[a] = np.where(has_b, np.where(has_a, np.where(mn[b] < mn[a], mn[b], mn[a]), mn[b]), mn[a])
            mx[a] = np.where(has_b, np.where(has_a, np.where(mx[b] > mx[a], mx[b], mx[a]), mx[b]), mx[a])
            n[a] = n[a] + n[b]
            lsum[a] = lsum[a] + lsum[b]
            s[a] = s[a] + s[b]
            ss[a] = ss[a] + ss[b]
            h //= 2
        return dict(episodes=int(n[0]), unfinished=int(self.remaining), length_sum=int(lsum[0]), sum=float(s[0]),
                    sumsq=float(ss[0]), min=np.float32(mn[0]), max=np.float32(mx[0]))


TABS = {1: np.array([0], np.int32),
        11: np.array([0, 1, 2, 3, 5, 7, 300, -4, 255, 256, 12], np.int32)}  # entries beyond the clamp on purpose

GRID = [(N, K, R) for N in (1, 63, 64, 65, 255, 256, 257, 1000) for K in (1, 3) for R in (1, 11)]
STEPS = 40


OVER_MODES = ('ones', 'zeros', 'random')
SUMMARY_AT = (0, 4, 19, STEPS - 1)  # the steps after which the summary is compared as well


def sequence(N, K, R, mode, steps=STEPS):
    """The test sequence of one grid point: per step (r_idx, reward, over). mode: over all ones (every
    env freezes after K steps), all zeros (nothing ever finishes) or random at p = 0.2 (some envs freeze
    early, some are still playing at the early summaries); r_idx leaves [0, R) on both sides."""
    rs = np.random.RandomState(1000003 * N + 101 * K + R)
    out = []
    for t in range(steps):
        r_idx = rs.randint(-3, R + 3, N).astype(np.int32)
        reward = rs.randint(-4, 5, N).astype(np.float32) * np.float32(0.37)
        if mode == 'ones':
            over = np.ones(N, np.float32)
        elif mode == 'zeros':
            over = np.zeros(N, np.float32)
        else:  # (any non-zero value ends an episode)
            over = (rs.rand(N) < 0.2).astype(np.float32) * np.float32(1 + t % 2)
        out.append((r_idx, reward, over))
    return out
