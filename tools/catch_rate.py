"""Throughput of the device-resident games (manette_amd/device_game.py), Catch by default.

  kernel   mt_catch_step alone at E = 32 / 64, gray / RGB, R = 1 / 11, as a hipGraph of back-to-back
           calls between device events (bench.graph_time), beside mt_preprocess_resized on the same
           shapes and push counts: the stack traffic is the same, the game logic and the renders are the
           difference.
  rollout  env-steps/s of the learner (NIPS, ec 32, T 5, rollout + update) with the rollout enqueued
           without a host synchronisation against the lockstep form (one after every step), the two
           alternating in one process, three rounds.

  graph    env-steps/s of the same learner under --iteration_graph (one replayed graph per iteration,
           drained every --drain_every) against the asynchronous eager path, two learners alternating in
           one process, three rounds; beside it the device time per iteration (K iterations captured as one
           graph between device events, bench.graph_time) and the wall time per iteration: the difference
           is the host gap that remains.

  python tools/catch_rate.py [--updates 300] [--skip_kernel] [--skip_rollout] [--skip_graph] [--game bricks]
One JSON line per measurement. --game bricks measures the device-resident Bricks (manette_amd/bricks.py) the
same way: its kernel lines carry bricks_step_us beside catch_step_us and preprocess_resized_us of the same run.
--game tetris (manette_amd/tetris.py) adds tetris_step_us to those lines.
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _tag(game):
    return {} if game == 'catch' else {'game': game}  # (the default's lines are what they were)


# what a --game run times, in this order, and the macro-steps each game plays first (catch: the yardstick's
# pushes; bricks: balls in play, the first nexts serve; tetris: some way into its episodes)
MEASURED = {'catch': ('catch',), 'bricks': ('catch', 'bricks'), 'tetris': ('catch', 'bricks', 'tetris')}
WARM_STEPS = {'catch': 1, 'bricks': 8, 'tetris': 40}


def kernel_times(inner=50, reps=5, game='catch'):
    import torch
    import bench
    from manette_amd import device_game, network as devnet
    games = device_game.games()
    for E in (32, 64):
        for depth in (1, 3):
            for R in (1, 11):
                tab = [0] if R == 1 else [i for i in range(11)]
                z = lambda *s, **k: torch.zeros(*s, device='cuda', **k)
                bufs = [z(E, 84, 84, 4 * depth, dtype=torch.uint8), z(E, 84, 84, 4 * depth, dtype=torch.uint8)]
                rs = np.random.RandomState(0)
                reward, over, rm = z(E), z(E), z(2, 1, E)
                frames, count = z(4 * E, 84, 84, depth, dtype=torch.uint8), z(E, dtype=torch.int32)
                off = torch.arange(0, 4 * E, 4, dtype=torch.int32, device='cuda')
                k = [0]

                def stack():
                    devnet.preprocess(frames, off, count, E, depth, None, None, bufs[k[0] & 1], bufs[1 - (k[0] & 1)],
                                      resized=True)
                    k[0] += 1

                us, r = {}, None
                for name in MEASURED[game]:  # the same buffers, repetition indices and table under every game
                    dev = games[name].Device(E, tab, seed=1, rgb=depth == 3)
                    a = torch.from_numpy(rs.randint(0, games[name].num_actions, E).astype(np.int32)).cuda()
                    if r is None:
                        r = torch.from_numpy(rs.randint(0, R, E).astype(np.int32)).cuda()
                    dev.reset(bufs[0])
                    for _ in range(WARM_STEPS[name]):
                        dev.step(a, r, bufs[0], bufs[1], reward, over, rm, 0, 1, frames, count)

                    def step():
                        dev.step(a, r, bufs[k[0] & 1], bufs[1 - (k[0] & 1)], reward, over, rm, 0, 1)
                        k[0] += 1

                    us[name + '_step'] = bench.graph_time(step, inner, reps)
                    if name == 'catch':  # beside mt_preprocess_resized on catch's frames and push counts
                        mean_pushes = float(count.float().mean())
                        us['preprocess_resized'] = bench.graph_time(stack, inner, reps)
                line = dict(what='kernel', **_tag(game), E=E, depth=depth, R=R)
                if game == 'catch':
                    line['mean_pushes'] = mean_pushes
                line.update({key + '_us': round(float(np.median(t)), 2) for key, t in us.items()})
                line.update({key + '_all': [round(x, 2) for x in t] for key, t in us.items()})
                print(json.dumps(line), flush=True)


def rollout_rates(updates=300, rounds=3, ec=32, game='catch'):
    import torch
    from catch_learn import make_learner
    with tempfile.TemporaryDirectory() as tmp:
        L = make_learner(tmp, 0, ec=ec, game=game)
        T = L.max_local_steps

        def run(lockstep, n):
            L.lockstep = lockstep
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                L.book.new_update()
                L.rollout()
                L.update()
            torch.cuda.synchronize()
            return n * T * ec / (time.perf_counter() - t0)

        run(False, 20)
        run(True, 20)
        res = []
        for _ in range(rounds):
            res.append((run(False, updates), run(True, updates)))
        L.cleanup()
    print(json.dumps(dict(what='rollout', **_tag(game), ec=ec, T=T, updates=updates,
                          async_steps_per_s=[round(a) for a, _ in res], lockstep_steps_per_s=[round(b) for _, b in res],
                          async_median=round(float(np.median([a for a, _ in res]))),
                          lockstep_median=round(float(np.median([b for _, b in res]))))), flush=True)


def graph_rates(updates=300, rounds=3, ec=32, drain_every=None, inner=8, reps=5, game='catch'):
    import torch
    import bench
    from catch_learn import make_learner
    with tempfile.TemporaryDirectory() as tmp:
        Le = make_learner(os.path.join(tmp, 'eager'), 0, ec=ec, game=game)
        Lg = make_learner(os.path.join(tmp, 'graph'), 0, ec=ec, iteration_graph=True, drain_every=drain_every, game=game)
        T, K = Le.max_local_steps, Lg.drain_every

        def eager(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                Le.book.new_update()
                Le.rollout()
                Le.update()
            torch.cuda.synchronize()
            return n * T * ec / (time.perf_counter() - t0)

        def graph(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            done = 0
            while done < n:
                k = min(K, n - done)
                for _ in range(k):
                    Lg.rollout()
                Lg.drain()
                done += k
            torch.cuda.synchronize()
            return n * T * ec / (time.perf_counter() - t0)

        eager(20)
        graph(20)
        res = []
        for _ in range(rounds):
            res.append((graph(updates), eager(updates)))
        assert inner * (reps + 1) <= K, 'the timed replays must fit the ring between two drains'
        dev_us = bench.graph_time(Lg._iteration_work, inner, reps)
        Lg.global_step += inner * (reps + 1) * T * ec  # (the mirror follows the timed iterations)
        Lg.drain()
        Le.cleanup()
        Lg.cleanup()
    wall_us = [1e6 * T * ec / g for g, _ in res]
    print(json.dumps(dict(what='graph', **_tag(game), ec=ec, T=T, updates=updates, drain_every=K,
                          graph_steps_per_s=[round(g) for g, _ in res], eager_steps_per_s=[round(e) for _, e in res],
                          graph_median=round(float(np.median([g for g, _ in res]))),
                          eager_median=round(float(np.median([e for _, e in res]))),
                          graph_not_slower_in_every_round=all(g >= e for g, e in res),
                          device_us_per_iteration=round(float(np.median(dev_us)), 1),
                          device_us_all=[round(x, 1) for x in dev_us],
                          wall_us_per_iteration=[round(x, 1) for x in wall_us])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--updates', type=int, default=300)
    ap.add_argument('--skip_kernel', action='store_true')
    ap.add_argument('--skip_rollout', action='store_true')
    ap.add_argument('--skip_graph', action='store_true')
    ap.add_argument('--drain_every', type=int, default=None)
    ap.add_argument('--game', choices=['catch', 'bricks', 'tetris'], default='catch')
    args = ap.parse_args()
    if not args.skip_kernel:
        kernel_times(game=args.game)
    if not args.skip_rollout:
        rollout_rates(args.updates, game=args.game)
    if not args.skip_graph:
        graph_rates(args.updates, drain_every=args.drain_every, game=args.game)


if __name__ == '__main__':
    main()
