"""Environment factory: environment_creator.py:4-30 interface.

ALE (ale_python_interface) is not installed in this image, so Atari games are served by the
synthetic stand-in with the game's ALE minimal-action-set size (what environment_creator.py:28
reads from the ROM; sizes below are ALE's minimal action sets, cross-checked where the
reference's pretrained checkpoints pin a head width). If ale_python_interface becomes
importable, an ALE-backed emulator can be plugged in behind the same create_environment().
"""
from .synthetic import SyntheticBank, SyntheticEmulator

MINIMAL_ACTIONS = {
    'pong': 6, 'breakout': 4, 'seaquest': 18, 'ms_pacman': 9, 'space_invaders': 6, 'beam_rider': 9,
    'qbert': 6, 'enduro': 9, 'asterix': 9, 'alien': 18, 'amidar': 10, 'assault': 7, 'asteroids': 14,
    'atlantis': 4, 'bank_heist': 18, 'battle_zone': 18, 'boxing': 18, 'centipede': 18,
    'chopper_command': 18, 'crazy_climber': 9, 'demon_attack': 6, 'freeway': 3, 'frostbite': 18,
    'gopher': 8, 'gravitar': 18, 'hero': 18, 'kangaroo': 18, 'krull': 18, 'montezuma_revenge': 18,
    'private_eye': 18, 'riverraid': 18, 'road_runner': 18, 'robotank': 18, 'star_gunner': 18,
    'time_pilot': 10, 'tutankham': 8, 'up_n_down': 6, 'venture': 18, 'video_pinball': 9,
    'wizard_of_wor': 10, 'zaxxon': 18,
}


# games with a device-resident environment (--runner device): the game lives in HBM, one kernel per macro-step
DEVICE_GAMES = ('catch', 'bricks')
# and the reference's own game with one (its rule is tetris.py's, not this project's)
REFERENCE_DEVICE_GAMES = ('tetris',)
ALL_DEVICE_GAMES = DEVICE_GAMES + REFERENCE_DEVICE_GAMES


def has_device_env(game):
    return str(game).lower() in ALL_DEVICE_GAMES


class EnvironmentCreator(object):
    def __init__(self, args):
        game = args.game.lower()
        if game.endswith('-v0'):
            raise NotImplementedError('gym emulators are out of scope (SURVEY.md §2)')
        self.game = game
        self.rgb = bool(getattr(args, 'rgb', False))
        self.rank_offset = int(getattr(args, 'env_id_offset', 0))
        if game == 'catch':
            # a real game (manette_amd/catch.py): the same rule on the host (CatchEmulator) and in HBM
            # (create_device_env), both keyed on (--seed, global env id)
            from . import catch
            self.num_actions = catch.NUM_ACTIONS
            self.catch_args = dict(seed=int(getattr(args, 'seed', 0)), rgb=self.rgb,
                                   lives=int(getattr(args, 'catch_lives', catch.DEFAULT_LIVES)),
                                   max_balls=int(getattr(args, 'catch_max_balls', catch.DEFAULT_MAX_BALLS)))
            self.create_environment = lambda i: catch.CatchEmulator(self.rank_offset + i, **self.catch_args)
            return
        if game == 'bricks':
            # the second real game (manette_amd/bricks.py), through the same two faces
            from . import bricks
            self.num_actions = bricks.NUM_ACTIONS
            self.bricks_args = dict(seed=int(getattr(args, 'seed', 0)), rgb=self.rgb,
                                    lives=int(getattr(args, 'bricks_lives', bricks.DEFAULT_LIVES)),
                                    max_nexts=int(getattr(args, 'bricks_max_nexts', bricks.DEFAULT_MAX_NEXTS)),
                                    serve_wait=int(getattr(args, 'bricks_serve_wait', bricks.DEFAULT_SERVE_WAIT)))
            self.create_environment = lambda i: bricks.BricksEmulator(self.rank_offset + i, **self.bricks_args)
            return
        if game == 'tetris':
            # the reference's own game (manette_amd/tetris.py), through the same two faces
            from . import tetris
            self.num_actions = tetris.NUM_ACTIONS
            wait = tetris.RANDOM_START_WAIT if getattr(args, 'random_start', False) else tetris.DEFAULT_MAX_START_WAIT
            self.tetris_args = dict(seed=int(getattr(args, 'seed', 0)), rgb=self.rgb,
                                    max_nexts=int(getattr(args, 'tetris_max_nexts', tetris.DEFAULT_MAX_NEXTS)),
                                    speed=int(getattr(args, 'tetris_speed', tetris.DEFAULT_SPEED)),
                                    max_start_wait=wait)
            self.create_environment = lambda i: tetris.TetrisEmulator(self.rank_offset + i, **self.tetris_args)
            return
        self.num_actions = MINIMAL_ACTIONS.get(game, 18)
        self.create_environment = lambda i: SyntheticEmulator(self.rank_offset + i, self.num_actions,
                                                              rgb=self.rgb)

    def create_device_env(self, n_envs, tab_rep, device='cuda'):
        """Envs [0, n_envs) of this rank (global ids offset by rank) as a device-resident environment."""
        if not has_device_env(self.game):
            raise ValueError('game %r has no device environment (--runner device serves: %s)'
                             % (self.game, ', '.join(ALL_DEVICE_GAMES)))
        if self.game == 'bricks':
            from . import bricks
            return bricks.BricksDevice(n_envs, tab_rep, env0=self.rank_offset, device=device, **self.bricks_args)
        if self.game == 'tetris':
            from . import tetris
            return tetris.TetrisDevice(n_envs, tab_rep, env0=self.rank_offset, device=device, **self.tetris_args)
        from . import catch
        return catch.CatchDevice(n_envs, tab_rep, env0=self.rank_offset, device=device, **self.catch_args)

    def create_bank(self, first_local, n_envs):
        """Native bank of envs [first_local, first_local+n) (global ids offset by rank)."""
        if self.game in ALL_DEVICE_GAMES:
            raise ValueError('game %r runs under --runner device or --runner python, not the native runner' % self.game)
        return SyntheticBank(self.rank_offset + first_local, n_envs, rgb=self.rgb)
