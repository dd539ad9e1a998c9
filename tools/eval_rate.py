"""Cost of the device-resident evaluation (manette_amd/evaluate.py).

  macro   device time of one evaluation macro-step (forward infer -> draw -> env kernel -> mt_eval_step,
          LSTM: + mt_memory_push) for a game, arch and n: blocks of two steps captured as one hipGraph
          between device events (bench.graph_time's method), per step.
  step    mt_eval_step alone at N = 64 and 4096, beside mt_book_rollout (T = 5, E = N) of the same run.
  wall    test.py's host loop against --runner device on the same checkpoint and n (both with -np 0, the
          multinomial chooser, one episode per env): three rounds, each in a process of its own that runs
          the host loop and then the device path; the times are whole test.run() calls, so both carry the
          same network creation and checkpoint restore.

  python tools/eval_rate.py [--game catch] [--arch NIPS] [--n 64] [--figar] [--rgb] [--skip_macro] [--skip_step]
                            [--skip_wall]
One JSON line per measurement.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def train_args(game, arch, figar, rgb, folder, ec=32):
    import train as cli
    a = cli.get_arg_parser().parse_args([])
    a.game, a.arch, a.rgb, a.emulator_counts, a.emulator_workers = game, arch, rgb, ec, 0
    a.runner, a.sampling, a.seed = 'device', 'device', 0
    a.max_repetition, a.nb_choices = (10, 11) if figar else (0, 1)
    a.debugging_folder = folder + '/'
    a.checkpoint_interval = 1 << 40
    return cli, a


def setup(game, arch, figar, rgb):
    from manette_amd.exploration_policy import ExplorationPolicy
    cli, a = train_args(game, arch, figar, rgb, tempfile.gettempdir())
    explo = ExplorationPolicy(a)
    nc, creator = cli.get_network_and_environment_creator(a, explo)
    net = nc()
    net.init_params(1)
    return net, creator, explo.tab_rep


def macro_step_time(game, arch, n, figar, rgb, inner=16, reps=5):
    import bench
    from manette_amd import evaluate
    net, creator, tab = setup(game, arch, figar, rgb)
    ev = evaluate.DeviceEvaluator(net, creator, tab, n, graph=False, max_macro_steps=8)
    ev.run()  # workspaces exist, games in play
    us = [t / 2 for t in bench.graph_time(lambda: ev._block(2), inner, reps)]
    print(json.dumps(dict(what='macro', game=game, arch=arch, n=n, figar=figar, rgb=rgb,
                          macro_step_us=round(float(np.median(us)), 2), all=[round(x, 2) for x in us])), flush=True)


def eval_step_time(inner=50, reps=5):
    import ctypes as C
    import bench
    import torch
    from manette_amd import _lib, evaluate
    from manette_amd.bookkeeping import DeviceBook
    from manette_amd.network import _ptr, _stream
    for N in (64, 4096):
        for R in (1, 11):
            K, T, A = 2, 5, 4
            tab = list(range(R))
            _, nbytes = evaluate.state_layout(N, K)
            block = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
            state = evaluate.make_state(block.data_ptr(), N, K)
            rs = np.random.RandomState(0)
            d = lambda x: torch.from_numpy(x).cuda()
            a = d(rs.randint(0, A, (T, N)).astype(np.int32))
            r = d(rs.randint(0, R, (T, N)).astype(np.int32))
            reward = d(rs.randint(-1, 2, (T, N)).astype(np.float32))
            over = d((rs.rand(T, N) < 0.05).astype(np.float32))
            tab_d = d(np.asarray(tab, np.int32))
            lib = _lib.hip()
            _lib.check(lib.mt_eval_reset(C.byref(state), _stream()))
            k = [0]

            def step():  # (K = 2 at p = 0.05: most envs freeze during the timed replays, as in a real run)
                t = k[0] % T
                _lib.check(lib.mt_eval_step(C.byref(state), _ptr(r[t]), _ptr(reward[t]), _ptr(over[t]), _ptr(tab_d), R,
                                            _stream()), 'mt_eval_step')
                k[0] += 1

            # (episode ends at p = 0.05: a quarter of the worst case holds every record of the timed replays)
            book = DeviceBook(N, A, tab, inner * (reps + 2) * T * N // 4, 0.0224, 8e7)
            t_eval = bench.graph_time(step, inner, reps)
            t_book = bench.graph_time(lambda: book.rollout(a, r, reward, over, T), inner, reps)
            t_sum = bench.graph_time(lambda: _lib.check(lib.mt_eval_summarize(
                C.byref(state), C.c_void_p(block.data_ptr() + 16), _stream())), inner, reps)
            print(json.dumps(dict(what='step', N=N, R=R, K=K, eval_step_us=round(float(np.median(t_eval)), 2),
                                  book_rollout_T5_us=round(float(np.median(t_book)), 2),
                                  eval_summarize_us=round(float(np.median(t_sum)), 2),
                                  eval_step_all=[round(x, 2) for x in t_eval],
                                  book_rollout_all=[round(x, 2) for x in t_book])), flush=True)


def make_checkpoint(game, arch, figar, rgb, folder, updates=20):
    """A short training run's checkpoint and args.json in `folder` (what test.py reads)."""
    from manette_amd import logger_utils
    from manette_amd.exploration_policy import ExplorationPolicy
    from manette_amd.paac import PAACLearner
    cli, a = train_args(game, arch, figar, rgb, folder)
    a.max_global_steps = updates * a.max_local_steps * a.emulator_counts
    cli.validate_args(a)
    logger_utils.save_args(a, a.debugging_folder)
    explo = ExplorationPolicy(a)
    nc, creator = cli.get_network_and_environment_creator(a, explo)
    PAACLearner(nc, creator, explo, a).train()


def wall_round(folder, n):
    """One round, in this process: the host loop, then the device path; one JSON line."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location('manette_test_cli', os.path.join(ROOT, 'test.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    out = {}
    for runner in ('host', 'device'):
        args = cli.get_arg_parser().parse_args(['-f', folder, '-tc', str(n), '-np', '0', '--runner', runner,
                                                '--draw_seed', '1'])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rewards = cli.run(args)
        torch.cuda.synchronize()
        out[runner + '_s'] = round(time.perf_counter() - t0, 4)
        out[runner + '_mean'] = round(float(np.mean(rewards)), 3)
    print('ROUND ' + json.dumps(out), flush=True)


def wall_times(game, arch, n, figar, rgb, rounds=3):
    with tempfile.TemporaryDirectory() as tmp:
        make_checkpoint(game, arch, figar, rgb, tmp)
        res = []
        for _ in range(rounds):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--wall_round', tmp, '--n', str(n)],
                               capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise RuntimeError('round failed: ' + p.stdout[-1000:] + p.stderr[-2000:])
            res.append(json.loads([l for l in p.stdout.splitlines() if l.startswith('ROUND ')][-1][6:]))
    print(json.dumps(dict(what='wall', game=game, arch=arch, n=n, figar=figar, rgb=rgb, rounds=res,
                          host_over_device=[round(r['host_s'] / r['device_s'], 2) for r in res],
                          device_not_slower_in_every_round=all(r['device_s'] <= r['host_s'] for r in res))),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--game', choices=['catch', 'bricks', 'tetris'], default='catch')
    ap.add_argument('--arch', default='NIPS')
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--figar', action='store_true')
    ap.add_argument('--rgb', action='store_true')
    ap.add_argument('--skip_macro', action='store_true')
    ap.add_argument('--skip_step', action='store_true')
    ap.add_argument('--skip_wall', action='store_true')
    ap.add_argument('--wall_round', default=None, help='(internal) one round on this folder')
    args = ap.parse_args()
    if args.wall_round:
        return wall_round(args.wall_round, args.n)
    if not args.skip_macro:
        macro_step_time(args.game, args.arch, args.n, args.figar, args.rgb)
    if not args.skip_step:
        eval_step_time()
    if not args.skip_wall:
        wall_times(args.game, args.arch, args.n, args.figar, args.rgb)


if __name__ == '__main__':
    main()
