"""Training CLI: the flags, defaults, args.json and signal handling of the reference's train.py
(train.py:1-130), driving the MI355X learner (manette_amd.paac.PAACLearner).

Extra flags (this build only): --runner {native,python,device}, --sampling {host,device},
--staging {resized,in_place,zero_copy,copy,pooled}, --no_pipeline, --seed, --bayes_native,
--catch_lives, --catch_max_balls (-g catch: the device-resident game, manette_amd/catch.py),
--bricks_lives, --bricks_max_nexts, --bricks_serve_wait (-g bricks: the second one, manette_amd/bricks.py),
--tetris_max_nexts, --tetris_speed (-g tetris: the reference's own game, manette_amd/tetris.py; --random_start gives
its new games up to 30 noop acts before their initial state),
--iteration_graph, --drain_every (the device game's whole iteration as one replayed graph),
--eval_every, --eval_envs, --eval_episodes, --eval_greedy (device-resident evaluation during training).
Multi-GPU: launch one process per GPU with torch.distributed.run; each rank trains
-ec emulators of its own (--ec_scope rank, the default) or -ec / WORLD_SIZE of them (--ec_scope
global: -ec 256 on 8 GPUs = 32 per GPU, BASELINE's "ec=256 sharded 8x32"); global env ids are
offset by rank, args.json records both counts, and gradients are all-reduced by RCCL behind the
C ABI (--comm rccl; torch.distributed runs on gloo as the control channel only).
Sampling: --sampling host (the default) draws with the reference's numpy multinomial stream
(exploration_policy.py:108-116, bit-exact parity with the reference); the benchmarked native
macro-step (bench.py) is --sampling device, which also takes --egreedy, --epsilon, --annealed and
--annealed_steps (the e-greedy draw and its annealing run in the heads kernel: mt_policy,
include/manette_hip.h).
"""
import argparse
import copy
import logging
import os
import signal
import sys

from manette_amd import logger_utils
from manette_amd.environment_creator import EnvironmentCreator
from manette_amd.exploration_policy import ExplorationPolicy

logging.basicConfig(stream=sys.stdout, level=logging.DEBUG)


def validate_args(args):
    """Flag combinations that are refused, before any device allocation."""
    from manette_amd.paac import check_arch_flags
    check_arch_flags(args)
    # --eval_*: device-resident evaluation during training (manette_amd/evaluate.py), off by default
    every, envs, episodes = (int(getattr(args, 'eval_every', 0)), int(getattr(args, 'eval_envs', 64)),
                             int(getattr(args, 'eval_episodes', 1)))
    if every < 0:
        raise ValueError('--eval_every must be >= 0 (0 = off), got %d' % every)
    if envs < 1 or episodes < 1:
        raise ValueError('--eval_envs and --eval_episodes must be >= 1, got %d and %d' % (envs, episodes))
    if every > 0 or getattr(args, 'eval_greedy', False):
        from manette_amd.environment_creator import ALL_DEVICE_GAMES, has_device_env
        if not has_device_env(getattr(args, 'game', 'pong')):
            raise ValueError('--eval_every / --eval_greedy evaluate in device memory and need a game with a device '
                             'environment (-g %s), got -g %s' % (' | '.join(ALL_DEVICE_GAMES), args.game))


def main(args):
    logging.debug('Configuration: {}'.format(args))
    validate_args(args)
    _setup_distributed(args)
    logger_utils.save_args(args, args.debugging_folder)  # (per rank: rank r > 0 writes under rank<r>/)
    if args.sampling == 'host':
        logging.info('--sampling host: the reference\'s numpy sampling stream (parity mode); '
                     '--sampling device runs the benchmarked native macro-step')
    explo_policy = ExplorationPolicy(args)
    print('Repetition table : ' + str(explo_policy.tab_rep))
    network_creator, env_creator = get_network_and_environment_creator(args, explo_policy)
    from manette_amd.paac import PAACLearner
    learner = PAACLearner(network_creator, env_creator, explo_policy, args)
    setup_kill_signal_handler(learner)
    logging.info('Starting training')
    learner.train()
    logging.info('Finished training')


def _setup_distributed(args):
    import torch
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if torch.cuda.is_available():
        torch.cuda.set_device(local)
    if world > 1 and not torch.distributed.is_initialized():
        # control channel only (RCCL unique id, resume step); the gradient goes over mt_allreduce
        torch.distributed.init_process_group('gloo')
    rank = torch.distributed.get_rank() if world > 1 else 0
    per_rank, offset = shard_emulators(args.emulator_counts, getattr(args, 'ec_scope', 'rank'), world, rank)
    args.emulator_counts = per_rank
    args.emulator_counts_per_rank = per_rank
    args.emulator_counts_global = per_rank * world
    args.world_size = world
    args.env_id_offset = offset
    if rank != 0:
        args.debugging_folder = os.path.join(args.debugging_folder, 'rank%d' % rank)


def shard_emulators(ec, scope, world, rank):
    """(emulators of this rank, global id of its first env): -ec per rank (scope 'rank') or for the
    whole job (scope 'global', split evenly); rank r owns the contiguous global ids
    [r * per_rank, (r + 1) * per_rank) — the np.split of runners.py:17-18 applied over ranks."""
    if scope == 'global':
        if ec % world:
            raise ValueError('-ec %d is not divisible by WORLD_SIZE %d' % (ec, world))
        ec //= world
    return ec, rank * ec


def setup_kill_signal_handler(learner):
    main_process_pid = os.getpid()

    def signal_handler(signal, frame):
        if os.getpid() == main_process_pid:
            logging.info('Signal ' + str(signal) + ' detected, cleaning up.')
            learner.cleanup()
            logging.info('Cleanup completed, shutting down...')
            sys.exit(0)

    signal.signal(signal.SIGTERM, signal_handler)
    signal.signal(signal.SIGINT, signal_handler)


def get_network_and_environment_creator(args, explo_policy, random_seed=3):
    env_creator = EnvironmentCreator(args)
    num_actions = env_creator.num_actions
    args.num_actions = num_actions
    args.random_seed = random_seed

    network_conf = {'num_actions': num_actions,
                    'entropy_regularisation_strength': args.entropy_regularisation_strength,
                    'device': args.device,
                    'clip_norm': args.clip_norm,
                    'clip_norm_type': args.clip_norm_type,
                    'softmax_temp': explo_policy.softmax_temp,
                    'keep_percentage': explo_policy.keep_percentage,
                    'rgb': args.rgb,
                    'activation': args.activation,
                    'alpha_leaky_relu': args.alpha_leaky_relu,
                    'max_repetition': args.max_repetition,
                    'nb_choices': args.nb_choices,
                    'arch': args.arch,
                    'alpha': args.alpha,
                    'e': args.e}

    def network_creator(name='local_learning'):
        from manette_amd.network import DeviceNetwork
        conf = copy.copy(network_conf)
        conf['name'] = name
        return DeviceNetwork(conf)

    return network_creator, env_creator


def get_arg_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('-g', default='pong', help='Name of game', dest='game')
    parser.add_argument('-d', '--device', default='/gpu:0', type=str, help="Device to be used ('/cpu:0', '/gpu:0', '/gpu:1',...)", dest="device")
    parser.add_argument('--rom_path', default='./atari_roms', help='Directory where the game roms are located (needed for ALE environment)', dest="rom_path")
    parser.add_argument('-v', '--visualize', default=0, type=int, help="0: no visualization of emulator; 1: all emulators, for all actors, are visualized; 2: only 1 emulator (for one of the actors) is visualized", dest="visualize")
    parser.add_argument('--e', default=0.1, type=float, help="Epsilon for the Rmsprop and Adam optimizers", dest="e")
    parser.add_argument('--alpha', default=0.99, type=float, help="Discount factor for the history/coming gradient, for the Rmsprop optimizer", dest="alpha")
    parser.add_argument('-lr', '--initial_lr', default=0.0224, type=float, help="Initial value for the learning rate. Default = 0.0224", dest="initial_lr")
    parser.add_argument('-lra', '--lr_annealing_steps', default=80000000, type=int, help="Nr. of global steps during which the learning rate will be linearly annealed towards zero", dest="lr_annealing_steps")
    parser.add_argument('--entropy', default=0.02, type=float, help="Strength of the entropy regularization term (needed for actor-critic)", dest="entropy_regularisation_strength")
    parser.add_argument('--clip_norm', default=3.0, type=float, help="If clip_norm_type is local/global, grads will be clipped at the specified maximum (avaerage) L2-norm", dest="clip_norm")
    parser.add_argument('--clip_norm_type', default="global", help="Whether to clip grads by their norm or not. Values: ignore (no clipping), local (layer-wise norm), global (global norm)", dest="clip_norm_type")
    parser.add_argument('--gamma', default=0.99, type=float, help="Discount factor", dest="gamma")
    parser.add_argument('--max_global_steps', default=80000000, type=int, help="Max. number of training steps", dest="max_global_steps")
    parser.add_argument('--max_local_steps', default=5, type=int, help="Number of steps to gain experience from before every update.", dest="max_local_steps")
    parser.add_argument('--arch', default='PWYX', help="Which network architecture to use: from the NIPS or NATURE paper, or PWYX, or LSTM, or BAYESIAN ie dropout", dest="arch")
    parser.add_argument('--single_life_episodes', action='store_true', help="If True, training episodes will be terminated when a life is lost (for games)", dest="single_life_episodes")
    parser.add_argument('-ec', '--emulator_counts', default=32, type=int, help="The amount of emulators per agent. Default is 32.", dest="emulator_counts")
    parser.add_argument('-ew', '--emulator_workers', default=8, type=int, help="The amount of emulator workers per agent. Default is 8.", dest="emulator_workers")
    parser.add_argument('-df', '--debugging_folder', default='logs/', type=str, help="Folder where to save the debugging information.", dest="debugging_folder")
    parser.add_argument('-rs', '--random_start', action='store_true', help="Whether or not to start with 30 noops for each env. Default True (-g tetris: each new game first plays up to 30 noop acts, drawn per game)", dest="random_start")
    parser.add_argument('--egreedy', action='store_true', help="If True, e-greedy policy is used to  choose actions", dest="egreedy")
    parser.add_argument('--epsilon', default=0.05, type=float, help="Epsilon for the egreedy policy", dest='epsilon')
    parser.add_argument('--softmax_temp', default=1.0, type=float, help="Softmax temperature for the Boltzmann action policy", dest='softmax_temp')
    parser.add_argument('--annealed', action='store_true', help="If True, the parameters for explo_policy are annealed toward zero", dest="annealed")
    parser.add_argument('--annealed_steps', default=80000000, type=int, help="Nb of global steps during which epsilon will be linearly annealed towards zero", dest="annealed_steps")
    parser.add_argument('--keep_percentage', default=0.9, type=float, help="keep percentage when dropout is used", dest='keep_percentage')
    parser.add_argument('--rgb', action='store_true', help="If True, RGB images are given to the agent", dest="rgb")
    parser.add_argument('--max_repetition', default=0, type=int, help="Maximum number of repetition for FiGAR", dest="max_repetition")
    parser.add_argument('--nb_choices', default=1, type=int, help="Number of possible repetitions", dest="nb_choices")
    parser.add_argument('--checkpoint_interval', default=1000000, type=int, help="Interval of steps btw checkpoints", dest="checkpoint_interval")
    parser.add_argument('--activation', default='relu', type=str, help="activation function for the network", dest="activation")
    parser.add_argument('--alpha_leaky_relu', default=0.1, type=float, help="coef for leaky relu", dest="alpha_leaky_relu")
    # this build
    parser.add_argument('--runner', default='native', choices=['native', 'python', 'device'], help='native: C++ emulator threads + GPU preprocess; python: reference-contract emulator processes; device: the game lives in HBM, one kernel per macro-step steps, renders and stacks it (-g catch, -g bricks or -g tetris; not --arch LSTM)', dest='runner')
    parser.add_argument('--tetris_max_nexts', default=2000, type=int, help='-g tetris: the cap on an episode\'s emulator steps (next() calls)', dest='tetris_max_nexts')
    parser.add_argument('--tetris_speed', default=5, type=int, help='-g tetris: acts per gravity drop at level 1 (the reference\'s 5)', dest='tetris_speed')
    parser.add_argument('--catch_lives', default=3, type=int, help='-g catch: misses that end an episode', dest='catch_lives')
    parser.add_argument('--catch_max_balls', default=20, type=int, help='-g catch: balls of an episode', dest='catch_max_balls')
    parser.add_argument('--bricks_lives', default=3, type=int, help='-g bricks: lost balls that end an episode', dest='bricks_lives')
    parser.add_argument('--bricks_max_nexts', default=500, type=int, help='-g bricks: the cap on an episode\'s emulator steps (next() calls)', dest='bricks_max_nexts')
    parser.add_argument('--bricks_serve_wait', default=4, type=int, help='-g bricks: emulator steps a parked ball waits for a fire action before it is served anyway', dest='bricks_serve_wait')
    parser.add_argument('--staging', default='resized', choices=['in_place', 'zero_copy', 'copy', 'pooled', 'resized'],
                        help='native runner screens: each push\'s final 84x84 frame pooled + resized by the emulator '
                             'threads and read in place from pinned memory (resized), the GPU reading the emulators\' '
                             'pinned bank (in_place), staged rows read in place (zero_copy, pooled = host frame-pool max) '
                             'or staged rows hipMemcpyAsync\'d (copy)',
                        dest='staging')
    parser.add_argument('--no_pipeline', action='store_false', help='native device-sampling step: do not enqueue '
                        'step t+1\'s preprocess + forward behind a device wait on a host step word '
                        '(MT_ROLLOUT_PIPELINED, on by default)', dest='pipeline')
    parser.add_argument('--sampling', default='host', choices=['host', 'device'], help='host (default): numpy multinomial, the reference\'s stream (parity mode); device: the draw fused into the heads kernel (multinomial, or e-greedy with --egreedy / --epsilon / --annealed / --annealed_steps), the benchmarked native macro-step', dest='sampling')
    parser.add_argument('--ec_scope', default='rank', choices=['rank', 'global'], help='data parallel: -ec emulators per rank (rank, the reference\'s meaning for one process) or for the whole job, split evenly over WORLD_SIZE ranks (global)', dest='ec_scope')
    parser.add_argument('--bayes_native', action='store_true', help='--arch BAYESIAN only: the native macro-step '
                        '(with --sampling device and the native runner) and the update as one captured graph around '
                        'the fused dropout backward (mt_dropout_returns_loss_backward); off: the Python step and the '
                        'eager update', dest='bayes_native')
    parser.add_argument('--iteration_graph', action='store_true', help='--runner device --sampling device only (one '
                        'process; NIPS / NATURE / PWYX): a whole training iteration (rollout, device bookkeeping '
                        'mt_book_rollout, update) as one graph replayed per iteration, with no host synchronisation '
                        'between drains; summaries, the log line and checkpoints land on drain boundaries',
                        dest='iteration_graph')
    parser.add_argument('--drain_every', default=None, type=int, help='--iteration_graph: iterations launched back to '
                        'back between two drains of the device book (default max(1, 2048 // ec), the logging interval)',
                        dest='drain_every')
    parser.add_argument('--eval_every', default=0, type=int, help='-g catch / -g bricks / -g tetris: every this many global steps '
                        '(0 = off) the chief plays --eval_envs x --eval_episodes fixed games in device memory with the '
                        'current parameters (manette_amd/evaluate.py) and writes eval/* scalars; also once at the end. '
                        'With --iteration_graph: at the first drain at or past the multiple', dest='eval_every')
    parser.add_argument('--eval_envs', default=64, type=int, help='--eval_every: envs of an evaluation', dest='eval_envs')
    parser.add_argument('--eval_episodes', default=1, type=int, help='--eval_every: episodes per env', dest='eval_episodes')
    parser.add_argument('--eval_greedy', action='store_true', help='--eval_every: evaluate the argmax policy (default: '
                        'the training chooser)', dest='eval_greedy')
    parser.add_argument('--seed', default=0, type=int, help='parameter init / device sampling seed', dest='seed')
    parser.add_argument('--comm', default='rccl', choices=['rccl', 'torch'], help='data-parallel gradient all-reduce: '
                        'rccl = RCCL behind the C ABI (mt_allreduce, one GPU per rank); torch = torch.distributed on '
                        'the process group (ranks sharing a GPU, tests)', dest='comm')
    parser.add_argument('--pin_threads', default='auto', choices=['auto', 'slice', 'pin', 'on', 'off'], help='native runner '
                        'thread placement (manette_amd/placement.py): pin the emulator threads and the host thread '
                        'to cores of the GPU\'s NUMA node, capping -ew when the node\'s cores are oversubscribed; '
                        'auto = only when several ranks share the node', dest='pin_threads')
    return parser


if __name__ == '__main__':
    args = get_arg_parser().parse_args()
    logging.debug(args)
    main(args)
