"""Learning curve of the device-resident Catch (manette_amd/catch.py): NIPS, --runner device --sampling
device, the hyper-parameters of the reference's pretrained/catcher run (lr 0.02 annealed over 3e8 steps,
entropy 0.02, clip 3, gamma 0.99, T 5, ec 32). Per seed: the mean return of the last 100 finished
episodes every --every updates, and the first update at which it reaches the bar = halfway between the
uniform-random policy's mean return (host restatement, no rendering) and max_balls. The run is
deterministic: counter-based draws, no float atomics. One JSON line per seed.

  python tools/catch_learn.py --seeds 0 1 2 --max_updates 20000

--game bricks: the same for the device-resident Bricks (manette_amd/bricks.py) at its default config, the bar
being 4 x the uniform-random policy's mean return (bricks_bar), and --max_seconds a wall-clock cap per seed.

--game tetris: the device-resident Tetris (manette_amd/tetris.py) at its default config. Under clipped rewards
the first thing to learn is that dropping pays, so the bar is on the reward per next(): the mean of return /
length over the last 100 finished episodes, against the midpoint between the uniform-random policy's value and
the always-drop policy's (tetris_bar).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def policy_mean(game, choose, episodes, seed, per_next=False, **cfg):
    """Mean return (per_next: mean of return / length) over `episodes` episodes of env 0 of `game` on its host
    face (mt_<game>_step_host, no rendering) under choose() -> action."""
    from manette_amd import device_game
    g = device_game.games()[game]
    c = g.config(**cfg)
    st = g.state_class()
    g.host_reset(c, seed, 0, 1, st)
    tab = np.zeros(1, np.int32)
    means, ret, n = [], 0.0, 0
    while len(means) < episodes:
        rw, over, _ = g.host_step(c, seed, 0, 1, tab, choose(), 0, st)
        ret += rw
        n += 1
        if over:
            means.append(ret / n if per_next else ret)
            ret, n = 0.0, 0
    return float(np.mean(means))


def _uniform(num_actions):
    rs = np.random.RandomState(12345)
    return lambda: int(rs.randint(num_actions))


def bar(lives, max_balls, episodes=100, seed=0):
    """Halfway between the uniform-random policy's mean return and max_balls."""
    return 0.5 * (policy_mean('catch', _uniform(3), episodes, seed, lives=lives, max_balls=max_balls) + max_balls)


def bricks_bar(episodes=100, seed=0, **cfg):
    """4 x the uniform-random policy's mean return."""
    return 4.0 * policy_mean('bricks', _uniform(4), episodes, seed, **cfg)


def tetris_policy_rate(choose, episodes=100, seed=0, **cfg):
    return policy_mean('tetris', choose, episodes, seed, per_next=True, **cfg)


def tetris_bar(episodes=100, seed=0, **cfg):
    """The midpoint between the uniform-random policy's reward per next and the always-drop policy's."""
    return 0.5 * (tetris_policy_rate(_uniform(5), episodes, seed, **cfg) +
                  tetris_policy_rate(lambda: 3, episodes, seed, **cfg))


def make_learner(folder, seed, ec=32, arch='NIPS', lives=3, max_balls=20, sampling='device', max_rep=0, nb=1,
                 iteration_graph=False, drain_every=None, game='catch', tetris_cfg=None):
    import train as cli
    from manette_amd.exploration_policy import ExplorationPolicy
    from manette_amd.paac import PAACLearner
    a = cli.get_arg_parser().parse_args([])
    a.game, a.arch, a.emulator_counts, a.emulator_workers = game, arch, ec, 0
    a.runner, a.sampling, a.seed = 'device', sampling, seed
    a.max_repetition, a.nb_choices = max_rep, nb
    a.catch_lives, a.catch_max_balls = lives, max_balls
    if tetris_cfg is not None:
        a.tetris_max_nexts, a.tetris_speed = tetris_cfg
    a.iteration_graph, a.drain_every = iteration_graph, drain_every
    a.initial_lr, a.lr_annealing_steps = 0.02, 300000000  # pretrained/catcher/args.json
    a.debugging_folder = folder + '/'
    a.max_global_steps = 1 << 40
    a.checkpoint_interval = 1 << 40
    explo = ExplorationPolicy(a)
    nc, ec_ = cli.get_network_and_environment_creator(a, explo)
    L = PAACLearner(nc, ec_, explo, a)
    L.start()
    return L


def train_until(L, target, max_updates, every=0, window=100, max_seconds=None, per_next=False):
    """Updates until the mean return (per_next: the mean of return / length) of the last `window` finished
    episodes >= target (checked after every update); returns (updates run, reached, curve [(update, mean)])."""
    curve = []
    t0 = time.time()
    for u in range(1, max_updates + 1):
        if max_seconds is not None and time.time() - t0 > max_seconds:
            return u - 1, False, curve
        L.book.new_update()
        L.rollout()
        L.update()
        if L.iteration_graph:  # (the bar is checked after every update: one drain each)
            L.drain()
        tr = L.book.total_rewards
        if per_next and len(tr) >= window:
            mean = float(np.mean(np.asarray(tr[-window:], np.float64) / np.asarray(L.book.total_steps[-window:])))
        else:
            mean = float(np.mean(tr[-window:])) if len(tr) >= window else None
        if every and u % every == 0:
            curve.append((u, mean))
        if mean is not None and mean >= target:
            curve.append((u, mean))
            return u, True, curve
    return max_updates, False, curve


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, nargs='+', default=[0, 1, 2])
    ap.add_argument('--max_updates', type=int, default=20000)
    ap.add_argument('--every', type=int, default=500)
    ap.add_argument('--ec', type=int, default=32)
    ap.add_argument('--lives', type=int, default=3)
    ap.add_argument('--max_balls', type=int, default=20)
    ap.add_argument('--game', choices=['catch', 'bricks', 'tetris'], default='catch')
    ap.add_argument('--max_seconds', type=float, default=None, help='stop a seed after this many seconds')
    ap.add_argument('--iteration_graph', action='store_true', help='train under --iteration_graph (drained after '
                    'every update, the bar being checked there): the arithmetic is the eager path\'s')
    args = ap.parse_args()
    import torch
    bricks_game = args.game == 'bricks'
    tetris_game = args.game == 'tetris'
    target = bricks_bar() if bricks_game else tetris_bar() if tetris_game else bar(args.lives, args.max_balls)
    for seed in args.seeds:
        with tempfile.TemporaryDirectory() as tmp:
            L = make_learner(tmp, seed, ec=args.ec, lives=args.lives, max_balls=args.max_balls, game=args.game,
                             iteration_graph=args.iteration_graph, drain_every=1 if args.iteration_graph else None)
            t0 = time.time()
            n, reached, curve = train_until(L, target, args.max_updates, args.every, max_seconds=args.max_seconds,
                                            per_next=tetris_game)
            torch.cuda.synchronize()
            dt = time.time() - t0
            L.cleanup()
        extra = {'iteration_graph': True} if args.iteration_graph else {}
        if bricks_game or tetris_game:
            extra['game'] = args.game
        print(json.dumps(dict(seed=seed, bar=target, reached=reached, updates=n, seconds=round(dt, 2), **extra,
                              env_steps=n * args.ec * 5, episodes=len(L.book.total_rewards),
                              curve=[(u, None if m is None else round(m, 3 if tetris_game else 2)) for u, m in curve])), flush=True)


if __name__ == '__main__':
    main()
