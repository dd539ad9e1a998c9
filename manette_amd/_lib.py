"""ctypes bindings of the two C-ABI libraries (include/manette_hip.h, include/manette_host.h).

The HIP library is the only compute path: if it is missing or fails to load, every device
call raises (there is no CPU fallback in the product).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB = os.environ.get('MANETTE_HIP_LIB') or os.path.join(HERE, 'libmanette_hip.so')  # variant override
HOST_LIB = os.path.join(HERE, 'libmanette_host.so')

MT_ARCH = {'NIPS': 0, 'NATURE': 1, 'PWYX': 2, 'LSTM': 3, 'BAYESIAN': 4}
MT_ACT = {'relu': 0, 'leaky_relu': 1}
MT_CLIP = {'ignore': 0, 'global': 1}
MT_NORM_PARTIALS = 512
MT_COMM_UID_BYTES = 128


class MTError(RuntimeError):
    pass


class mt_rollout_buffers(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('states', 'values', 'idx', 'pi', 'rep', 'ws')] + \
               [('ws_bytes', C.c_size_t)] + \
               [(n, C.c_void_p) for n in ('counters', 'raw')] + [('src_rows', C.c_int32)] + \
               [(n, C.c_void_p) for n in ('pair', 'pair_host', 'meta', 'row_lut', 'col_lut', 'idx_host',
                                          'staging_host', 'meta_host', 'reward_host', 'over_host',
                                          'rm_host', 'frames_host', 'sync_host', 'train_ws')] + \
               [('train_ws_bytes', C.c_size_t), ('v_boot', C.c_void_p), ('ready_host', C.c_void_p), ('flags', C.c_int32),
                                                                       ('env_offset', C.c_int32), ('nz', C.c_void_p)]


MT_ROLLOUT_ZERO_COPY = 1
MT_ROLLOUT_IN_PLACE = 2
MT_ROLLOUT_POOLED = 4
MT_ROLLOUT_PIPELINED = 8
MT_ROLLOUT_RESIZED = 16
MT_ROLLOUT_BOOT_SLABS = 32
MT_ROLLOUT_DROPOUT = 64
MH_RUNNER_RESIZED = 4
MH_RUNNER_FIXED_SLOTS = 1
MH_RUNNER_POOLED = 2


class mt_net_config(C.Structure):
    _fields_ = [('arch', C.c_int32), ('depth', C.c_int32), ('num_actions', C.c_int32),
                ('num_reps', C.c_int32), ('activation', C.c_int32), ('alpha_leaky', C.c_float),
                ('softmax_temp', C.c_float), ('keep_prob', C.c_float)]


MT_POLICY = {'multinomial': 0, 'egreedy': 1, 'argmax': 2}


class mt_policy(C.Structure):
    """Exploration policy of the device draw (include/manette_hip.h); all zeros = multinomial."""
    _fields_ = [('mode', C.c_int32), ('annealed', C.c_int32), ('epsilon', C.c_double),
                ('annealing_steps', C.c_double), ('rows_per_call', C.c_int64)]


class mt_catch_config(C.Structure):
    """Catch (include/manette_hip.h): lives and balls of an episode."""
    _fields_ = [('lives', C.c_int32), ('max_balls', C.c_int32)]


class mt_catch_state(C.Structure):
    """Per-env Catch state, 32 bytes."""
    _fields_ = [(n, C.c_int32) for n in ('paddle_x', 'ball_x', 'ball_y', 'ball_dx', 'misses', 'balls')] + \
               [('ball_counter', C.c_uint64)]


class mt_bricks_config(C.Structure):
    """Bricks (include/manette_hip.h): lives, the cap on an episode's nexts, nexts a parked ball waits."""
    _fields_ = [('lives', C.c_int32), ('max_nexts', C.c_int32), ('serve_wait', C.c_int32)]


class mt_bricks_state(C.Structure):
    """Per-env Bricks state, 56 bytes."""
    _fields_ = [(n, C.c_int32) for n in ('paddle_x', 'ball_x', 'ball_y', 'ball_dx', 'ball_dy', 'lives', 'nexts',
                                         'wait')] + \
               [('bricks_lo', C.c_uint64), ('bricks_hi', C.c_uint32), ('reserved', C.c_uint32),
                ('serve_counter', C.c_uint64)]


class mt_tetris_config(C.Structure):
    """Tetris (include/manette_hip.h): the cap on an episode's nexts, the acts per gravity drop at level 1,
    the most noop acts before a game's initial state."""
    _fields_ = [('max_nexts', C.c_int32), ('speed', C.c_int32), ('max_start_wait', C.c_int32)]


class mt_tetris_state(C.Structure):
    """Per-env Tetris state, 136 bytes."""
    _fields_ = [('board', C.c_uint32 * 22)] + \
               [(n, C.c_int32) for n in ('piece', 'rot', 'x', 'y', 'next_piece', 'level', 'lines', 'speed',
                                         'speed_counter', 'nexts')] + \
               [('piece_counter', C.c_uint64)]


class mt_book_words(C.Structure):
    """The device book's word block (include/manette_hip.h, "Device bookkeeping"), 40 bytes."""
    _fields_ = [(n, C.c_int64) for n in ('global_step', 'written', 'acked', 'nb_actions')] + \
               [('overflow', C.c_int32), ('reserved', C.c_int32)]


class mt_book_episode(C.Structure):
    """One episode record of the device book's ring, 24 bytes."""
    _fields_ = [('global_step', C.c_int64), ('length', C.c_int64), ('reward', C.c_float), ('reserved', C.c_int32)]


class mt_book_state(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('total_episode_rewards', 'emulator_steps', 'words', 'hist', 'lr', 'ring')] + \
               [('capacity', C.c_int64)]


class mt_eval_words(C.Structure):
    """The device evaluation's word block (include/manette_hip.h, "Device evaluation"), 16 bytes."""
    _fields_ = [('remaining', C.c_int64), ('steps', C.c_int64)]


class mt_eval_state(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('ret_acc', 'len_acc', 'done', 'returns', 'lengths', 'words')] + \
               [('N', C.c_int32), ('K', C.c_int32)]


class mt_eval_summary(C.Structure):
    """What mt_eval_summarize writes, 56 bytes."""
    _fields_ = [(n, C.c_int64) for n in ('episodes', 'unfinished', 'length_sum')] + \
               [('sum', C.c_double), ('sumsq', C.c_double), ('min', C.c_float), ('max', C.c_float),
                ('pad', C.c_int32 * 2)]


_P = C.c_void_p
_I = C.c_int
_F = C.c_float
_SZ = C.c_size_t

_HIP_SIGS = {
    'mt_last_error': (C.c_char_p, []),
    'mt_version': (_I, []),
    'mt_launch_window': (_I, [_I, _I]),
    'mt_net_backward_bucket_launches': (_I, [_P, C.POINTER(_I)]),
    'mt_net_create': (_I, [C.POINTER(mt_net_config), C.POINTER(_P)]),
    'mt_net_destroy': (None, [_P]),
    'mt_net_num_params': (_I, [_P, C.POINTER(_SZ)]),
    'mt_net_num_vars': (_I, [_P, C.POINTER(_I)]),
    'mt_net_var_info': (_I, [_P, _I, C.c_char_p, _I, C.POINTER(C.c_int64), C.POINTER(_I),
                             C.POINTER(_SZ), C.POINTER(_F)]),
    'mt_net_feature_dim': (_I, [_P, C.POINTER(_I)]),
    'mt_net_workspace_bytes': (_I, [_P, _I, C.POINTER(_SZ)]),
    'mt_net_workspace_region': (_I, [_P, _I, _I, _I, _I, _I, C.POINTER(_SZ), C.POINTER(_SZ)]),
    'mt_forward': (_I, [_P, _P, _P, _I, _P, _SZ, _P, _P, _P, _P]),
    'mt_lstm_frames_workspace_bytes': (_I, [_P, _I, _I, C.POINTER(_SZ)]),
    'mt_lstm_frames_forward': (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _SZ, _P]),
    'mt_lstm_windows_forward': (_I, [_P, _P, _P, _I, _I, _I, _P, _SZ, _P, _P, _P, _P]),
    'mt_lstm_step_forward': (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _SZ, _P, _P, _P, _P]),
    'mt_lstm_frames_backward': (_I, [_P, _P, _P, _P, _I, _I, _P, _SZ, _P, _P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P]),
    'mt_forward_rows': (_I, [_P, _P, _P, _I, _P, _SZ, _P, _SZ, _I, _I, _P, _P, _P, _P]),
    'mt_forward_trunk': (_I, [_P, _P, _P, _I, _P, _SZ, _P]),
    'mt_forward_trunk_stacking': (_I, [_P, _P, _P, _P, _P, C.c_uint32, _P, _I, _P, _SZ, _P, _P]),
    'mt_forward_infer': (_I, [_P, _P, _P, _I, _P, _SZ, _P, _P, _P, _P]),
    'mt_sample': (_I, [_P, _P, _I, _I, _I, C.c_uint64, _I, _P, _P, _P, _P, _P]),
    'mt_sample_policy': (_I, [C.POINTER(mt_policy), _P, _P, _I, _I, _I, C.c_uint64, _I, _P, _P, _P, _P, _P]),
    'mt_policy_draw_host': (_I, [C.POINTER(mt_policy), C.c_uint64, C.c_uint64, C.c_uint64, _P, _I, _P, _I,
                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'mt_rollout_set_policy': (_I, [_P, C.POINTER(mt_policy)]),
    'mt_returns': (_I, [_P, _P, _P, _P, C.c_double, _I, _I, _P, _P, _P]),
    'mt_loss_backward': (_I, [_P, _P, _P, _I, _P, _SZ, _P, _P, _P, _P, _P, _P, _P, _F, _P, _P, _P]),
    'mt_dropout_redraw': (_I, [_P, _P, _I, _P, _SZ, _P, _P, _P, _P]),
    'mt_dropout_returns_loss_backward': (_I, [_P, _P, _P, _I, _I, _P, _SZ, _P, _P, _P, _P, _P, _P, C.c_double, _P, _P,
                                              _P, _P, _P, _F, _P, _P, _P, _P]),
    'mt_dropout_mask_host': (_I, [C.c_uint64, C.c_uint64, C.c_uint64, _F, _P]),
    'mt_returns_loss_backward': (_I, [_P, _P, _P, _I, _I, _P, _SZ, _P, _P, _P, _P, _P, _P, _P, _P, C.c_double, _P, _P,
                                      _F, _P, _P, _P, _P]),
    'mt_returns_loss_backward_boot': (_I, [_P, _P, _P, _I, _I, _P, _SZ, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _P,
                                           C.c_double, _P, _P, _F, _P, _P, _P, _P]),
    'mt_grad_sumsq': (_I, [_P, _SZ, _F, _P, _P]),
    'mt_clip_rmsprop': (_I, [_P, _P, _P, _P, _SZ, _P, _P, _F, _F, _F, _F, _I, _F, _P, _P]),
    'mt_preprocess': (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    'mt_preprocess_pooled': (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    'mt_preprocess_resized': (_I, [_P, _P, _P, _I, _I, _P, _P, _P]),
    'mt_preprocess_frames': (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
    'mt_memory_push': (_I, [_P, _P, _P, _P, _I, _SZ, _P]),
    'mt_host_device_pointer': (_I, [_P, C.POINTER(_P)]),
    'mt_sum_slabs': (_I, [_P, _I, _SZ, _P, _P]),
    'mt_net_get_config': (_I, [_P, C.POINTER(mt_net_config)]),
    'mt_rollout_create': (_I, [_P, _I, _I, _P, _P, C.POINTER(mt_rollout_buffers), C.c_uint64, C.POINTER(_P)]),
    'mt_rollout_destroy': (None, [_P]),
    'mt_rollout_step': (_I, [_P, _P, _I, C.POINTER(C.c_int64), _P]),
    'mt_rollout_run': (_I, [_P, _P, C.POINTER(C.c_int64), _P]),
    'mt_rollout_stats': (_I, [_P, C.POINTER(C.c_double), _I]),
    'mt_rollout_stats_ex': (_I, [_P, _P, _I, _I]),
    'mt_rollout_host_trace': (_I, [_P, _P, _I, _P]),
    'mt_rollout_trunk_timing': (_I, [_P, _I, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'mt_rollout_set_update': (_I, [_P, _P, _P, C.c_double, C.c_double]),
    'mt_rollout_update_form': (_I, [_P, C.POINTER(_I)]),
    'mt_rollout_set_update_dp': (_I, [_P, _P, _P, _P, _SZ, _SZ, _P, C.c_double, C.c_double]),
    'mt_comm_unique_id': (_I, [C.c_char_p]),
    'mt_comm_init': (_I, [C.c_char_p, _I, _I, _I, C.POINTER(_P)]),
    'mt_comm_init_loopback': (_I, [_I, _I, C.POINTER(_P)]),
    'mt_comm_destroy': (None, [_P]),
    'mt_comm_info': (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    'mt_allreduce': (_I, [_P, _P, _SZ, _P]),
    'mt_broadcast': (_I, [_P, _P, _SZ, _I, _P]),
    'mt_graph_begin': (_I, [_P]),
    'mt_graph_end': (_I, [_P, C.POINTER(_P)]),
    'mt_graph_launch': (_I, [_P, _P]),
    'mt_graph_destroy': (_I, [_P]),
    'mt_book_rollout': (_I, [C.POINTER(mt_book_state), _P, _P, _P, _P, _P, _I, _I, _I, _I, C.c_int64, C.c_int64,
                             C.c_double, C.c_double, _P]),
    'mt_book_rollout_host': (_I, [C.POINTER(mt_book_state), _P, _P, _P, _P, _P, _I, _I, _I, _I, C.c_int64, C.c_int64,
                                  C.c_double, C.c_double]),
    'mt_eval_reset': (_I, [C.POINTER(mt_eval_state), _P]),
    'mt_eval_step': (_I, [C.POINTER(mt_eval_state), _P, _P, _P, _P, _I, _P]),
    'mt_eval_summarize': (_I, [C.POINTER(mt_eval_state), _P, _P]),
    'mt_eval_reset_host': (_I, [C.POINTER(mt_eval_state)]),
    'mt_eval_step_host': (_I, [C.POINTER(mt_eval_state), _P, _P, _P, _P, _I]),
    'mt_eval_summarize_host': (_I, [C.POINTER(mt_eval_state), _P]),
}

# The device games (include/manette_hip.h: "Catch", "Bricks", "Tetris") share one contract: four entry points
# each, whose signatures differ in the game's config and state structs only.
GAME_ENTRY_POINTS = ('reset', 'step', 'reset_host', 'step_host')
for _game, _cfg, _state in (('catch', mt_catch_config, mt_catch_state), ('bricks', mt_bricks_config, mt_bricks_state),
                            ('tetris', mt_tetris_config, mt_tetris_state)):
    _head = [C.POINTER(_cfg), C.c_uint64]
    _HIP_SIGS.update({
        'mt_%s_reset' % _game: (_I, _head + [_I, _I, _I, _P, _P, _P]),
        'mt_%s_step' % _game: (_I, _head + [_I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
        'mt_%s_reset_host' % _game: (_I, _head + [C.c_uint64, _I, C.POINTER(_state), _P]),
        'mt_%s_step_host' % _game: (_I, _head + [C.c_uint64, _I, _P, _I, _I, _I, C.POINTER(_state), _P, _P, _P,
                                                 C.POINTER(C.c_int32), C.POINTER(_F), C.POINTER(_F)]),
    })

_HOST_SIGS = {
    'mh_last_error': (C.c_char_p, []),
    'mh_runner_create': (_I, [_I, _I, _P, _I, _P, _I, _SZ, _P, _I, _I, _P, _I, _I, C.POINTER(_P)]),
    'mh_runner_destroy': (None, [_P]),
    'mh_runner_reset': (_I, [_P, _P, _P, _P, C.POINTER(_I)]),
    'mh_runner_step': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(_I)]),
    'mh_runner_reset_frames': (_I, [_P, _P, _P]),
    'mh_runner_step_frames': (_I, [_P, _P, _P, _P, _P, _P, _P]),
    'mh_runner_env_state': (_I, [_P, _I, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    'mh_crc32c': (C.c_uint32, [_P, _SZ, C.c_uint32]),
    'mh_runner_set_col_lut': (_I, [_P, _P, _I]),
    'mh_runner_set_threads': (_I, [_P, _P, _I, _I]),
    'mh_runner_thread_cpus': (_I, [_P, _P, _I]),
    'mh_runner_stats': (_I, [_P, _P, _I, _I]),
    'mh_runner_set_ready': (_I, [_P, _P, C.c_uint32]),
    'mh_runner_step_begin': (_I, [_P, _P, _P, _P, _P, _P, _P, _P]),
    'mh_runner_step_end': (_I, [_P, C.POINTER(_I)]),
    'mh_book_create': (_I, [_I, _I, _P, _I, C.POINTER(_P)]),
    'mh_book_destroy': (None, [_P]),
    'mh_book_step': (_I, [_P, C.POINTER(C.c_int64), _P, _P, _P, _P, _P, _P]),
    'mh_book_new_update': (_I, [_P]),
    'mh_book_set_shard': (_I, [_P, C.c_int64, C.c_int64]),
    'mh_book_histogram': (_I, [_P, _P, C.POINTER(C.c_int64)]),
    'mh_book_pop_episodes': (_I, [_P, _P, _P, _P, _I, C.POINTER(_I)]),
}

_hip = None
_host = None


def _load(path, sigs):
    if not os.path.exists(path):
        raise MTError('%s is not built (run __graft_entry__.build() or python -m manette_amd.build)'
                      % path)
    lib = C.CDLL(path)
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def hip():
    global _hip
    if _hip is None:
        host()  # libmanette_hip.so links libmanette_host.so (rpath $ORIGIN)
        _hip = _load(HIP_LIB, _HIP_SIGS)
    return _hip


def host():
    global _host
    if _host is None:
        _host = _load(HOST_LIB, _HOST_SIGS)
    return _host


def check(rc, what='call'):
    if rc != 0:
        msg = hip().mt_last_error()
        raise MTError('%s failed (status %d): %s' % (what, rc, msg.decode() if msg else ''))


def check_host(rc, what='call'):
    if rc != 0:
        msg = host().mh_last_error()
        raise MTError('%s failed (status %d): %s' % (what, rc, msg.decode() if msg else ''))


def hip_symbols():
    return sorted(_HIP_SIGS)


def host_symbols():
    return sorted(_HOST_SIGS)
