// Device bookkeeping of one rollout (include/manette_hip.h, "Device bookkeeping"): Bookkeeper.step for
// t = 0 .. T-1 as one kernel, so a rollout of a device-resident game leaves global_step, its episode
// records, its histogram and the LR of its update in device memory and the host need not wait for it.
#include "common.h"

namespace mt {

constexpr int BOOK_BLOCK = 256;
constexpr int BOOK_WAVES = BOOK_BLOCK / 64;

struct BookArgs {
  mt_book_state b;
  const int32_t *a_idx, *r_idx;
  const float *reward, *over;
  const int32_t *tab_rep;
  int A, R, E, T;
  int64_t env_offset, envs_total;
  double initial_lr, annealing_steps;
};

__host__ __device__ inline int book_clamp(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// Ring slot of record k: unsigned, so a corrupted (negative) count still lands inside the ring
__host__ __device__ inline int64_t book_slot(int64_t k, int64_t capacity) {
  return (int64_t)((uint64_t)k % (uint64_t)capacity);
}

// actor_learner.py:get_lr: a product, a quotient, a difference in double, rounded once to float
// (rollout.hip restates the same for the native step)
__host__ __device__ inline float book_lr(int64_t global_step, double initial_lr, double annealing_steps) {
  const double g = (double)global_step;
  const double lr = g <= annealing_steps ? initial_lr - (g * initial_lr / annealing_steps) : 0.0;
  return (float)lr;
}

// One workgroup. Pass 1 counts the rollout's episode ends (ballot + popcount per wave, the waves' counts
// summed through LDS), which decides whether its records fit the ring. Pass 2 walks t in order and the
// envs in chunks of the block, in order: a record's slot is the count so far + the ends of the earlier
// waves of its chunk (LDS) + the ends of the lower lanes of its wave (ballot). A thread meets the same
// envs at every t, so the accumulators it carries through global memory need no barrier. The LDS
// counters alternate between two rows: one barrier per chunk. Then one histogram cell per thread.
__global__ __launch_bounds__(BOOK_BLOCK) void book_kernel(BookArgs p) {
  __shared__ int wave_cnt[2][BOOK_WAVES];
  __shared__ long long red[BOOK_BLOCK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = p.E, T = p.T, R = p.R, A = p.A;
  const int64_t N = (int64_t)T * E;
  // (read by every thread here, written by thread 0 after the last barrier)
  const int64_t gs0 = p.b.words->global_step, written0 = p.b.words->written, acked = p.b.words->acked;
  const int32_t overflow0 = p.b.words->overflow;

  int ends = 0;  // wave-uniform
  for (int64_t i0 = 0; i0 < N; i0 += BOOK_BLOCK) {
    const int64_t i = i0 + tid;
    const bool o = i < N && p.over[i] != 0.f;
    ends += __popcll(__ballot(o));
  }
  if (lane == 0) wave_cnt[0][wave] = ends;
  __syncthreads();
  int64_t total = 0;
#pragma unroll
  for (int w = 0; w < BOOK_WAVES; ++w) total += wave_cnt[0][w];
  const bool fits = written0 + total - acked <= p.b.capacity;

  int par = 1;
  int64_t count = 0;  // records of this rollout so far (block-uniform)
  for (int t = 0; t < T; ++t) {
    const int64_t gs = gs0 + (int64_t)t * p.envs_total + p.env_offset;
    for (int c0 = 0; c0 < E; c0 += BOOK_BLOCK) {
      const int e = c0 + tid;
      const bool live = e < E;
      bool ended = false;
      float tot = 0.f;
      int64_t steps = 0;
      if (live) {
        const int64_t i = (int64_t)t * E + e;
        const int r = book_clamp(p.r_idx[i], R);
        tot = p.b.total_episode_rewards[e] + p.reward[i];
        steps = p.b.emulator_steps[e] + (int64_t)p.tab_rep[r] + 1;
        ended = p.over[i] != 0.f;
      }
      const unsigned long long mask = __ballot(ended);
      if (lane == 0) wave_cnt[par][wave] = __popcll(mask);
      __syncthreads();
      int before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < BOOK_WAVES; ++w) {
        const int c = wave_cnt[par][w];
        before += w < wave ? c : 0;
        all += c;
      }
      if (live) {
        if (ended) {
          if (fits) {
            const int64_t k = written0 + count + before + __popcll(mask & ((1ull << lane) - 1ull));
            mt_book_episode *rec = p.b.ring + book_slot(k, p.b.capacity);
            rec->global_step = gs + e + 1;
            rec->length = steps;
            rec->reward = tot;
            rec->reserved = 0;
          }
          tot = 0.f;
          steps = 0;
        }
        p.b.total_episode_rewards[e] = tot;
        p.b.emulator_steps[e] = steps;
      }
      count += all;
      par ^= 1;
    }
  }

  long long nb = 0;
  for (int cell = tid; cell < A * R; cell += BOOK_BLOCK) {
    const int a = cell / R, r = cell - a * R;
    long long n = 0;
    for (int64_t i = 0; i < N; ++i)
      n += (book_clamp(p.a_idx[i], A) == a && book_clamp(p.r_idx[i], R) == r) ? 1 : 0;
    p.b.hist[cell] = n;
    nb += n * (r + 1);
  }
  red[tid] = nb;
  __syncthreads();
  for (int s = BOOK_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t gs = gs0 + (int64_t)T * p.envs_total;
    p.b.words->global_step = gs;
    p.b.words->written = written0 + (fits ? total : 0);
    p.b.words->nb_actions = red[0];
    p.b.words->overflow = overflow0 | (fits ? 0 : 1);
    *p.b.lr = book_lr(gs, p.initial_lr, p.annealing_steps);
  }
}

static int book_check(const BookArgs &p, const char *who) {
  const mt_book_state &b = p.b;
  MT_CHECK_ARG(b.total_episode_rewards && b.emulator_steps && b.words && b.hist && b.lr && b.ring,
               "%s: null pointer in the book state", who);
  MT_CHECK_ARG(p.a_idx && p.r_idx && p.reward && p.over && p.tab_rep, "%s: null argument", who);
  MT_CHECK_ARG(p.A >= 1 && p.R >= 1 && p.E >= 1 && p.T >= 1, "%s: A, R, E and T must be >= 1", who);
  MT_CHECK_ARG((int64_t)p.A * p.R <= (int64_t)1 << 30, "%s: A * R too large", who);
  MT_CHECK_ARG(b.capacity >= 1, "%s: ring capacity must be >= 1", who);
  MT_CHECK_ARG(p.env_offset >= 0 && p.envs_total >= p.env_offset + p.E,
               "%s: the shard [env_offset, env_offset + E) must lie in [0, envs_total)", who);
  MT_CHECK_ARG(p.annealing_steps > 0.0, "%s: lr_annealing_steps must be > 0", who);
  return MT_OK;
}

}  // namespace mt

using namespace mt;

extern "C" int mt_book_rollout(const mt_book_state *book, const int32_t *a_idx, const int32_t *r_idx,
                               const float *reward, const float *over, const int32_t *tab_rep, int A, int R, int E,
                               int T, int64_t env_offset, int64_t envs_total, double initial_lr,
                               double lr_annealing_steps, mt_stream_t stream) {
  MT_CHECK_ARG(book != nullptr, "mt_book_rollout: null book");
  const BookArgs p = {*book, a_idx, r_idx, reward, over, tab_rep, A, R, E, T, env_offset, envs_total, initial_lr,
                      lr_annealing_steps};
  if (int rc = book_check(p, "mt_book_rollout")) return rc;
  MT_CHECK_ARG((((uintptr_t)book->emulator_steps | (uintptr_t)book->words | (uintptr_t)book->hist |
                 (uintptr_t)book->ring) & 7) == 0, "mt_book_rollout: misaligned buffer");
  hipLaunchKernelGGL(book_kernel, dim3(1), dim3(BOOK_BLOCK), 0, (hipStream_t)stream, p);
  MT_LAUNCHED();
  return MT_OK;
}

extern "C" int mt_book_rollout_host(const mt_book_state *book, const int32_t *a_idx, const int32_t *r_idx,
                                    const float *reward, const float *over, const int32_t *tab_rep, int A, int R,
                                    int E, int T, int64_t env_offset, int64_t envs_total, double initial_lr,
                                    double lr_annealing_steps) {
  MT_CHECK_ARG(book != nullptr, "mt_book_rollout_host: null book");
  const BookArgs p = {*book, a_idx, r_idx, reward, over, tab_rep, A, R, E, T, env_offset, envs_total, initial_lr,
                      lr_annealing_steps};
  if (int rc = book_check(p, "mt_book_rollout_host")) return rc;
  const mt_book_state &b = p.b;
  mt_book_words &w = *b.words;
  const int64_t N = (int64_t)T * E;
  int64_t total = 0;
  for (int64_t i = 0; i < N; ++i) total += over[i] != 0.f ? 1 : 0;
  const bool fits = w.written + total - w.acked <= b.capacity;
  int64_t k = w.written;
  for (int64_t i = 0; i < (int64_t)A * R; ++i) b.hist[i] = 0;
  int64_t nb = 0;
  for (int t = 0; t < T; ++t) {
    for (int e = 0; e < E; ++e) {
      const int64_t i = (int64_t)t * E + e;
      const int a = book_clamp(a_idx[i], A), r = book_clamp(r_idx[i], R);
      b.total_episode_rewards[e] += reward[i];
      b.emulator_steps[e] += (int64_t)tab_rep[r] + 1;
      b.hist[(int64_t)a * R + r] += 1;
      nb += r + 1;
      if (over[i] != 0.f) {
        if (fits) {
          mt_book_episode &rec = b.ring[book_slot(k, b.capacity)];
          rec.global_step = w.global_step + env_offset + e + 1;
          rec.length = b.emulator_steps[e];
          rec.reward = b.total_episode_rewards[e];
          rec.reserved = 0;
          ++k;
        }
        b.total_episode_rewards[e] = 0.f;
        b.emulator_steps[e] = 0;
      }
    }
    w.global_step += envs_total;
  }
  w.written = k;
  w.nb_actions = nb;
  if (!fits) w.overflow = 1;
  *b.lr = book_lr(w.global_step, initial_lr, lr_annealing_steps);
  return MT_OK;
}
