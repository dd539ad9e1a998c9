"""Per-step rollout bookkeeping (A8), vectorised over the env axis: paac.py:154-205.

Exact integer semantics of the reference loop:
  rewards[t] = clip(summed reward, +-1)                      (:180, actor_learner.py:108-114)
  masks[t] = 1 - over                                        (:176)
  emulator_steps[e] += tab_rep[r_e] + 1 (planned repeats)   (:183)
  global_step += 1 per env, in env order                    (:184)
  total_action_rep[a_e][r_e] += 1; nb_actions += r_e + 1     (:157, :187-189)
  on over: log (global_step at env e, total reward, emulator_steps), reset both   (:191-201)
Total episode rewards accumulate in float32 (the shared reward array is float32).
Data parallel (set_shard): a rank's envs are global envs [env_offset, env_offset + E) of a learner
stepping envs_total envs per macro-step; global_step then advances by envs_total (the same on
every rank) and episode records carry the global env's position, as one process would log them.
"""
import numpy as np


class Bookkeeper(object):
    def __init__(self, n_envs, num_actions, tab_rep):
        self.E = n_envs
        self.tab = np.asarray(tab_rep, dtype=np.int64)
        self.R = len(tab_rep)
        self.A = num_actions
        self.emulator_steps = np.zeros(n_envs, dtype=np.int64)
        self.total_episode_rewards = np.zeros(n_envs, dtype=np.float32)
        self.total_rewards = []
        self.total_steps = []
        self.episodes = []   # (global_step, reward, length)
        self.env_offset, self.envs_total = 0, n_envs
        self.new_update()

    def set_shard(self, env_offset, envs_total):
        assert 0 <= env_offset and env_offset + self.E <= envs_total
        self.env_offset, self.envs_total = int(env_offset), int(envs_total)

    def new_update(self):
        self.total_action_rep = np.zeros((self.A, self.R), dtype=np.int64)
        self.nb_actions = 0

    def step(self, global_step, a_idx, r_idx, reward, over, rewards_out, masks_out):
        """Returns the new global_step; fills rewards_out/masks_out (float32 views) in place."""
        a_idx = np.asarray(a_idx, dtype=np.int64)
        r_idx = np.asarray(r_idx, dtype=np.int64)
        reward = np.asarray(reward, dtype=np.float32)
        over = np.asarray(over)
        masks_out[...] = 1.0 - over.astype(np.float32)
        self.total_episode_rewards += reward
        rewards_out[...] = np.clip(reward, -1.0, 1.0)
        self.emulator_steps += self.tab[r_idx] + 1
        np.add.at(self.total_action_rep, (a_idx, r_idx), 1)
        self.nb_actions += int((r_idx + 1).sum())
        ended = np.nonzero(over)[0]
        for e in ended:
            self.total_rewards.append(float(self.total_episode_rewards[e]))
            self.total_steps.append(int(self.emulator_steps[e]))
            self.episodes.append((global_step + self.env_offset + int(e) + 1, float(self.total_episode_rewards[e]),
                                  int(self.emulator_steps[e])))
        self.total_episode_rewards[ended] = 0
        self.emulator_steps[ended] = 0
        return global_step + self.envs_total

    def histograms(self):
        """paac.py:269-275: the values log_histogram would receive."""
        nb_a = self.total_action_rep.sum(1)
        nb_r = self.total_action_rep.sum(0)
        histo_a = np.repeat(np.arange(self.A), nb_a)
        histo_r = np.repeat(self.tab + 1, nb_r)
        return histo_a, histo_r


class NativeBook(object):
    """The same bookkeeping in libmanette_host.so (mh_book_*), used by the learner so a native
    macro-step needs no Python; interface of Bookkeeper (tests pin one against the other)."""

    def __init__(self, n_envs, num_actions, tab_rep):
        import ctypes as C
        from . import _lib
        self._C = C
        self._lib = _lib
        self.E = n_envs
        self.A = num_actions
        self.tab = np.ascontiguousarray(np.asarray(tab_rep, dtype=np.int32))
        self.R = len(self.tab)
        h = C.c_void_p()
        _lib.check_host(_lib.host().mh_book_create(n_envs, num_actions, self.tab.ctypes.data_as(C.c_void_p),
                                                   self.R, C.byref(h)), 'mh_book_create')
        self._h = h
        self.total_rewards = []
        self.total_steps = []
        self.episodes = []

    def set_shard(self, env_offset, envs_total):
        self._lib.check_host(self._lib.host().mh_book_set_shard(self._h, int(env_offset), int(envs_total)),
                             'mh_book_set_shard')

    @property
    def handle(self):
        return self._h

    def step(self, global_step, a_idx, r_idx, reward, over, rewards_out, masks_out):
        C = self._C
        gs = C.c_int64(global_step)
        arrs = [np.ascontiguousarray(a_idx, np.int32), np.ascontiguousarray(r_idx, np.int32),
                np.ascontiguousarray(reward, np.float32), np.ascontiguousarray(over, np.float32)]
        assert rewards_out.flags.c_contiguous and masks_out.flags.c_contiguous
        self._lib.check_host(self._lib.host().mh_book_step(
            self._h, C.byref(gs), *[a.ctypes.data_as(C.c_void_p) for a in arrs],
            rewards_out.ctypes.data_as(C.c_void_p), masks_out.ctypes.data_as(C.c_void_p)), 'mh_book_step')
        self.drain()
        return gs.value

    def drain(self):
        C = self._C
        n = C.c_int(1)
        while n.value:
            st = np.zeros(256, np.int64)
            rw = np.zeros(256, np.float32)
            ln = np.zeros(256, np.int64)
            self._lib.check_host(self._lib.host().mh_book_pop_episodes(
                self._h, st.ctypes.data_as(C.c_void_p), rw.ctypes.data_as(C.c_void_p),
                ln.ctypes.data_as(C.c_void_p), 256, C.byref(n)))
            for i in range(n.value):
                self.total_rewards.append(float(rw[i]))
                self.total_steps.append(int(ln[i]))
                self.episodes.append((int(st[i]), float(rw[i]), int(ln[i])))

    def new_update(self):
        self._lib.check_host(self._lib.host().mh_book_new_update(self._h))

    def histograms(self):
        C = self._C
        hist = np.zeros((self.A, self.R), np.int64)
        nb = C.c_int64()
        self._lib.check_host(self._lib.host().mh_book_histogram(self._h, hist.ctypes.data_as(C.c_void_p),
                                                                C.byref(nb)))
        self.nb_actions = nb.value
        return np.repeat(np.arange(self.A), hist.sum(1)), np.repeat(self.tab.astype(np.int64) + 1, hist.sum(0))

    def __del__(self):
        h = getattr(self, '_h', None)
        if h:
            self._lib.host().mh_book_destroy(h)
            self._h = None


WORDS_DTYPE = np.dtype([('global_step', np.int64), ('written', np.int64), ('acked', np.int64),
                        ('nb_actions', np.int64), ('overflow', np.int32), ('reserved', np.int32)])
EPISODE_DTYPE = np.dtype([('global_step', np.int64), ('length', np.int64), ('reward', np.float32),
                          ('reserved', np.int32)])


class DeviceBook(object):
    """The same bookkeeping in device memory, advanced one rollout at a time by mt_book_rollout
    (include/manette_hip.h, "Device bookkeeping"): global_step, the episode ring, the last rollout's
    histogram and the LR word the RMSProp kernel reads, so nothing of a rollout has to reach the host
    before its update. Interface of Bookkeeper / NativeBook, minus step(); the host sees episodes,
    histograms and global_step as of the last drain().

    One allocation holds [words 40 B | lr 4 B | pad | hist A*R int64 | ring capacity x 24 B], so a drain is
    one D2H copy; the per-env accumulators stay on the device."""

    HIST_OFF = 48

    def __init__(self, n_envs, num_actions, tab_rep, capacity, initial_lr, lr_annealing_steps, device='cuda',
                 event=None):
        import torch
        from . import _lib
        self._lib = _lib
        self.E, self.A = int(n_envs), int(num_actions)
        self.tab = np.ascontiguousarray(np.asarray(tab_rep, dtype=np.int32))
        self.R = len(self.tab)
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError('DeviceBook: ring capacity must be >= 1')
        self.initial_lr, self.lr_annealing_steps = float(initial_lr), float(lr_annealing_steps)
        self.env_offset, self.envs_total = 0, self.E
        self.ring_off = self.HIST_OFF + 8 * self.A * self.R
        nbytes = self.ring_off + EPISODE_DTYPE.itemsize * self.capacity
        self.block = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self._pin = torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True)
        self._w64 = self.block[:32].view(torch.int64)  # global_step, written, acked, nb_actions
        self.lr = self.block[40:44].view(torch.float32)
        self.total_episode_rewards = torch.zeros(self.E, dtype=torch.float32, device=device)
        self.emulator_steps = torch.zeros(self.E, dtype=torch.int64, device=device)
        self.tab_d = torch.from_numpy(self.tab).to(device)
        base = self.block.data_ptr()
        self.lr_addr = base + 40
        self.state = _lib.mt_book_state(self.total_episode_rewards.data_ptr(), self.emulator_steps.data_ptr(), base,
                                        base + self.HIST_OFF, self.lr_addr, base + self.ring_off, self.capacity)
        self.event = event if event is not None else torch.cuda.Event()
        self.total_rewards = []
        self.total_steps = []
        self.episodes = []
        self.global_step = 0  # as of the last drain
        self.nb_actions = 0
        self.total_action_rep = np.zeros((self.A, self.R), dtype=np.int64)

    def set_shard(self, env_offset, envs_total):
        assert 0 <= env_offset and env_offset + self.E <= envs_total
        self.env_offset, self.envs_total = int(env_offset), int(envs_total)

    def set_global_step(self, global_step):
        """The device word at the start of a run (a resumed checkpoint's step), in stream order."""
        self._w64[0:1].fill_(int(global_step))
        self.global_step = int(global_step)

    def new_update(self):
        pass  # the kernel writes, not accumulates, its own rollout's histogram

    def rollout(self, a_idx, r_idx, reward, over, T):
        """mt_book_rollout over [T][E] device tensors, enqueued on the current stream (no sync)."""
        import ctypes as C
        from .network import _ptr, _stream
        self._lib.check(self._lib.hip().mt_book_rollout(
            C.byref(self.state), _ptr(a_idx), _ptr(r_idx), _ptr(reward), _ptr(over), _ptr(self.tab_d), self.A, self.R,
            self.E, int(T), self.env_offset, self.envs_total, self.initial_lr, self.lr_annealing_steps, _stream()),
            'mt_book_rollout')

    def drain(self):
        """One D2H copy of the block, acked = written in stream order, one synchronisation; appends the
        records [acked, written), raises on overflow, returns the device global_step."""
        self._pin.copy_(self.block, non_blocking=True)
        self._w64[2:3].copy_(self._w64[1:2])
        self.event.record()
        self.event.synchronize()
        host = self._pin.numpy()
        w = host[:WORDS_DTYPE.itemsize].view(WORDS_DTYPE)[0]
        if w['overflow']:
            raise self._lib.MTError('device book: the episode ring (capacity %d) overflowed; records were dropped'
                                    % self.capacity)
        ring = host[self.ring_off:].view(EPISODE_DTYPE)
        for k in range(int(w['acked']), int(w['written'])):
            rec = ring[k % self.capacity]
            self.total_rewards.append(float(rec['reward']))
            self.total_steps.append(int(rec['length']))
            self.episodes.append((int(rec['global_step']), float(rec['reward']), int(rec['length'])))
        self.total_action_rep = host[self.HIST_OFF:self.ring_off].view(np.int64).reshape(self.A, self.R).copy()
        self.nb_actions = int(w['nb_actions'])
        self.lr_value = np.float32(host[40:44].view(np.float32)[0])
        self.global_step = int(w['global_step'])
        return self.global_step

    def histograms(self):
        """Of the last rollout before the last drain (paac.py:269-275)."""
        hist = self.total_action_rep
        return np.repeat(np.arange(self.A), hist.sum(1)), np.repeat(self.tab.astype(np.int64) + 1, hist.sum(0))
