#!/usr/bin/env python
"""Env-steps/s of the BAYESIAN learner (bench.py's config table has no BAYESIAN line): synthetic Pong,
ec = 32, ew = 8, t_max = 5, keep 0.9, built the way tests/test_bayes_learner_gpu.py builds its learner.

  --mode python   --arch BAYESIAN without --bayes_native: Python step + eager update (mt_returns,
                  mt_dropout_redraw, mt_loss_backward, mt_grad_sumsq, mt_clip_rmsprop)
  --mode native   --arch BAYESIAN --bayes_native: native pipelined macro-step, captured fused update
  --mode nips     --arch NIPS on the native path (the yardstick)

Settles, warms up, times --updates updates between two host clock reads around a device sync and
prints one JSON line: env-steps/s, the emulator time per macro-step, the host phases of the native
step, and (with --update-timing) the update alone, K launches back to back between device events:
the captured graph where there is one, else the eager sequence.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_learner(mode, folder, ec=32, ew=8, t_max=5, keep=0.9, seed=0):
    import train as cli
    from manette_amd.exploration_policy import ExplorationPolicy
    from manette_amd.paac import PAACLearner
    argv = {'python': ['--arch', 'BAYESIAN'], 'native': ['--arch', 'BAYESIAN', '--bayes_native'],
            'nips': ['--arch', 'NIPS']}[mode]
    a = cli.get_arg_parser().parse_args(argv)
    a.game, a.emulator_counts, a.emulator_workers, a.max_local_steps = 'pong', ec, ew, t_max
    a.keep_percentage = keep
    a.runner, a.sampling, a.seed, a.staging, a.pipeline = 'native', 'device', seed, 'resized', True
    a.debugging_folder = folder
    a.max_global_steps = 1 << 40
    a.checkpoint_interval = 1 << 40
    np.random.seed(1234)
    explo = ExplorationPolicy(a)
    nc, ecr = cli.get_network_and_environment_creator(a, explo)
    L = PAACLearner(nc, ecr, explo, a)
    L.is_chief = False  # no checkpoint writes
    L.start()
    return L


def one_update(L):
    L.book.new_update()
    L.rollout()
    L.update()


def time_update(L, k):
    """The update alone, k times back to back between two device events (us per update)."""
    import torch
    from manette_amd import network as devnet
    s = devnet._stream()
    if L._graphs is not None and len(L._graphs) == 1:
        run, form = (lambda: L._launch_graph(L._graphs[0], s)), 'graph'
    else:
        def run():
            L._update_backward()
            L._update_apply()
        form = 'eager'
    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        run()
    e1.record()
    e1.synchronize()
    return form, 1e3 * e0.elapsed_time(e1) / k


def main():
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['python', 'native', 'nips'], required=True)
    ap.add_argument('--updates', type=int, default=400)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--settle', type=float, default=1.0, help='seconds of untimed updates first')
    ap.add_argument('--update-timing', type=int, default=0, metavar='K', help='also time K updates alone')
    o = ap.parse_args()
    import torch
    from manette_amd import _lib
    with tempfile.TemporaryDirectory() as tmp:
        L = make_learner(o.mode, tmp + '/')
        try:
            E, T = L.emulator_counts, L.max_local_steps
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < o.settle:
                one_update(L)
            for _ in range(o.warmup):
                one_update(L)
            torch.cuda.synchronize()
            emu = [0.0, 0]
            if L.native_step is not None:
                st = (C.c_double * 5)()
                _lib.check(_lib.hip().mt_rollout_stats(L.native_step, st, 1), 'mt_rollout_stats')
            else:  # the Python step: clock the runner's step call
                step = L.runners.step

                def timed(*a, **k):
                    c0 = time.perf_counter()
                    r = step(*a, **k)
                    emu[0] += 1e6 * (time.perf_counter() - c0)
                    emu[1] += 1
                    return r
                L.runners.step = timed
            c0 = time.perf_counter()
            for _ in range(o.updates):
                one_update(L)
            torch.cuda.synchronize()
            dt = time.perf_counter() - c0
            res = dict(mode=o.mode, ec=E, t_max=T, updates=o.updates, env_steps_per_s=o.updates * E * T / dt,
                       us_per_update=1e6 * dt / o.updates, native_step=L.native_step is not None,
                       update_graphs=0 if L._graphs is None else len(L._graphs),
                       update_in_rollout=bool(L._update_in_rollout))
            if L.native_step is not None:
                _lib.check(_lib.hip().mt_rollout_stats(L.native_step, st, 0), 'mt_rollout_stats')
                n = max(st[4], 1.0)
                res.update(emulator_us_per_step=st[1] / n, launch_and_wait_us=st[0] / n, book_us=st[2] / n,
                           enqueue_us=st[3] / n)
            else:
                res.update(emulator_us_per_step=emu[0] / max(emu[1], 1))
            if o.update_timing > 0:
                form, us = time_update(L, o.update_timing)
                # the launches mt_launch_window numbers in one eager backward (the loss kernel and the
                # grouped launches; the redraw's two and mt_returns are not numbered)
                lib = _lib.hip()
                lib.mt_launch_window(0, -1)
                try:
                    L._update_backward()
                finally:
                    numbered = lib.mt_launch_window(-1, -1)
                torch.cuda.synchronize()
                res.update(update_form=form, update_us=us, backward_numbered_launches=numbered)
            print(json.dumps(res))
        finally:
            L.cleanup()


if __name__ == '__main__':
    main()
