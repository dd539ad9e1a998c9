"""Regenerates tests/golden/tetris_rule.npz from the reference's own Tetris rule, on the CPU:

    python tests/golden/make_golden_tetris.py --reference <directory holding the reference's tetris.py>

The reference's tetris.py is imported unmodified with `pygame` replaced by a permissive stub module (the
rule, tetris.py:88-119, 147-170, 213-335, is pure integer list logic; only drawing goes to pygame) and
`scipy.misc.imsave` by a no-op, and its `rand` by this project's counter-based piece stream (tests/tetris_ref.py:
mix64 under the Tetris salt at a recorded (seed, global env)), so that mt_tetris_step_host can be replayed
against the recording act by act. The file holds recorded data only (actions, rewards, boards, pieces,
counters): nothing of the reference's text.

Traces: episodes played as tetris_emulator.py plays them (init_game() after a game over, then four act(0) for
the initial state: recorded with init = 1) under a uniform-random policy, an always-drop policy and the scripted
placement policy of tests/tetris_ref.py. Cases: every crafted state of tests/tetris_cases.py set into the
app's fields, one act, the result recorded."""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tetris_cases  # noqa: E402
import tetris_ref  # noqa: E402


class _Stub(object):
    """Anything pygame is asked for: callable, iterable as a size, usable as an integer."""

    def __call__(self, *a, **k):
        return _Stub()

    def __getattr__(self, name):
        return _Stub()

    def __iter__(self):
        return iter((0, 0))

    def __add__(self, other):
        return 0

    __radd__ = __add__


def load_reference(path):
    saved = {k: sys.modules.get(k) for k in ('pygame', 'scipy', 'scipy.misc', 'tetris')}
    pg = types.ModuleType('pygame')
    pg.__getattr__ = lambda name: _Stub()
    sp, spm = types.ModuleType('scipy'), types.ModuleType('scipy.misc')
    spm.imsave = lambda *a, **k: None
    sp.misc = spm
    sys.modules.update({'pygame': pg, 'scipy': sp, 'scipy.misc': spm})
    sys.modules.pop('tetris', None)
    sys.path.insert(0, path)
    try:
        import tetris
    finally:
        sys.path.remove(path)
        for k, v in saved.items():
            if k != 'tetris':
                if v is None:
                    sys.modules.pop(k, None)
                else:
                    sys.modules[k] = v
    return tetris


class Stream(object):
    def __init__(self, seed, env):
        self.seed, self.env, self.counter = seed, env, 0

    def rand(self, n):
        assert n == 7
        v = tetris_ref.piece_draw(self.seed, self.env, self.counter)
        self.counter += 1
        return int(v)


def shape_id(m):
    return max(max(row) for row in m)


class Recorder(object):
    KEYS = ('action', 'reward', 'gameover', 'init', 'board', 'stone', 'stone_h', 'stone_w', 'x', 'y', 'next_piece', 'level',
            'lines', 'speed', 'speed_counter', 'piece_counter')

    def __init__(self):
        self.rows = {k: [] for k in self.KEYS}

    def add(self, app, stream, action, reward, init):
        r = self.rows
        stone = np.zeros((4, 4), np.uint8)
        for y, row in enumerate(app.stone):
            stone[y, :len(row)] = row
        r['action'].append(action)
        r['reward'].append(reward)
        r['gameover'].append(int(bool(app.gameover)))
        r['init'].append(init)
        r['board'].append(np.asarray(app.board[:22], np.uint8))
        r['stone'].append(stone)
        r['stone_h'].append(len(app.stone))
        r['stone_w'].append(len(app.stone[0]))
        r['x'].append(app.stone_x)
        r['y'].append(app.stone_y)
        r['next_piece'].append(shape_id(app.next_stone))
        for k in ('level', 'lines', 'speed', 'speed_counter'):
            r[k].append(getattr(app, k))
        r['piece_counter'].append(stream.counter)

    def arrays(self, prefix):
        small = dict(board=np.uint8, stone=np.uint8, action=np.int8, gameover=np.uint8, init=np.uint8)
        return {prefix + k: np.asarray(v, small.get(k, np.int32)) for k, v in self.rows.items()}


def play(tetris, rec, seed, env, policy, episodes, max_acts):
    """Returns the number of recorded acts."""
    stream = Stream(seed, env)
    tetris.rand = stream.rand
    app = tetris.TetrisApp(emulator=True)
    n0 = len(rec.rows['action'])

    def initial():
        for _ in range(4):
            rw = app.act(0)
            rec.add(app, stream, 0, rw, 1)

    initial()
    done = 0
    while done < episodes and len(rec.rows['action']) - n0 < max_acts:
        a = policy(app, stream)
        rw = app.act(a)
        rec.add(app, stream, a, rw, 0)
        if app.gameover:
            done += 1
            app.init_game()
            initial()
    return len(rec.rows['action']) - n0


def save_npz(path, arrays):
    """np.savez_compressed's format with fixed member times and order, so the file regenerates byte for byte."""
    import io
    import zipfile
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='directory of the reference checkout (tetris.py)')
    ap.add_argument('--out', default=os.path.join(HERE, 'tetris_rule.npz'))
    args = ap.parse_args()
    tetris = load_reference(os.path.abspath(args.reference))

    rs = np.random.RandomState(20240607)
    placer = tetris_ref.PlacementPolicy()

    def scripted(app, stream):
        piece = shape_id(app.stone)
        return placer.action(stream.counter, app.board[:22], piece, tetris_ref.rot_of(piece, app.stone), app.stone_x,
                             app.stone_y)

    plans = [('random', 0x1234567, 0, lambda app, s: int(rs.randint(5)), 2, 2500),
             ('random', 0x1234567, 41, lambda app, s: int(rs.randint(5)), 1, 1500),
             ('drop', 77, 5, lambda app, s: 3, 3, 1000),
             ('scripted', 2024, 1, scripted, 1, 1800),
             ('scripted', 9, 1 << 20, scripted, 1, 1200)]
    rec = Recorder()
    starts, seeds, envs, names = [0], [], [], []
    for name, seed, env, policy, episodes, max_acts in plans:
        n = play(tetris, rec, seed, env, policy, episodes, max_acts)
        starts.append(starts[-1] + n)
        seeds.append(seed)
        envs.append(env)
        names.append(name)
    out = rec.arrays('t_')
    out.update(trace_start=np.asarray(starts, np.int64), trace_seed=np.asarray(seeds, np.uint64),
               trace_env=np.asarray(envs, np.uint64), trace_name=np.asarray(names))

    # crafted single acts
    pre, post = Recorder(), Recorder()
    stream = Stream(tetris_cases.SEED, tetris_cases.ENV)
    tetris.rand = stream.rand
    app = tetris.TetrisApp(emulator=True)
    for name, s, action in tetris_cases.CASES:
        app.board = [list(row) for row in s['board']] + [[1] * 10]
        app.stone = tetris_ref.matrix(s['piece'], s['rot'])
        app.next_stone = tetris.tetris_shapes[s['next_piece'] - 1]
        app.stone_x, app.stone_y = s['x'], s['y']
        app.level, app.lines, app.speed, app.speed_counter = s['level'], s['lines'], s['speed'], s['speed_counter']
        app.score, app.gameover, app.paused = 0, False, False
        stream.counter = s['piece_counter']
        pre.add(app, stream, action, 0, 0)
        rw = app.act(action)
        post.add(app, stream, action, rw, 0)
    out.update(post.arrays('case_'))
    out.update({'casepre_' + k: v for k, v in pre.arrays('').items() if k in ('board', 'stone', 'x', 'y')})
    out['case_name'] = np.asarray([c[0] for c in tetris_cases.CASES])
    save_npz(args.out, out)
    print('%s: %d acts in %d traces, %d cases, %d bytes' % (args.out, starts[-1], len(plans), len(tetris_cases.CASES),
                                                           os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
