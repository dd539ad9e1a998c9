// Device evaluation (include/manette_hip.h, "Device evaluation"): K episodes on each of N envs of a
// device-resident game, recorded where the env kernel ran. mt_eval_step follows every env kernel and
// keeps the per-episode return and length of the first K episodes of each env, freezing an env after
// its K-th; the word block tells the host how many episodes are still owed, so it looks once per block
// of macro-steps and not at every step. mt_eval_summarize reduces the tables in a fixed order.
#include "common.h"

namespace mt {

constexpr int EVAL_BLOCK = 256;

struct EvalStepArgs {
  mt_eval_state s;
  const int32_t *r_idx;
  const float *reward, *over;
  const int32_t *tab_rep;
  int R;
};

__host__ __device__ inline int eval_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The planned nexts of a macro-step that drew repetition index r: the env kernels' clamps
__host__ __device__ inline int64_t eval_nexts(const int32_t *tab_rep, int r, int R) {
  return (int64_t)eval_clamp(tab_rep[eval_clamp(r, 0, R - 1)], 0, 255) + 1;
}

// One env's step rule; returns K - done[e] after it (what this env still owes)
__host__ __device__ inline int64_t eval_step_env(const EvalStepArgs &p, int e) {
  const mt_eval_state &s = p.s;
  int32_t done = s.done[e];
  if (done >= 0 && done < s.K) {
    float ret = s.ret_acc[e] + p.reward[e];
    int64_t len = s.len_acc[e] + eval_nexts(p.tab_rep, p.r_idx[e], p.R);
    if (p.over[e] != 0.f) {
      const int64_t i = (int64_t)e * s.K + done;
      s.returns[i] = ret;
      s.lengths[i] = len;
      s.done[e] = ++done;
      ret = 0.f;
      len = 0;
    }
    s.ret_acc[e] = ret;
    s.len_acc[e] = len;
  }
  // (a corrupted count outside [0, K] owes nothing and writes nothing)
  return done >= 0 && done < s.K ? (int64_t)(s.K - done) : 0;
}

// Integer sum of the block's 256 partials through LDS; the result in red[0]
__device__ inline void eval_block_sum(long long *red, int tid) {
  __syncthreads();
  for (int s = EVAL_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
}

__global__ __launch_bounds__(EVAL_BLOCK) void eval_reset_kernel(mt_eval_state s) {
  const int tid = threadIdx.x;
  const int64_t NK = (int64_t)s.N * s.K;
  for (int e = tid; e < s.N; e += EVAL_BLOCK) {
    s.ret_acc[e] = 0.f;
    s.len_acc[e] = 0;
    s.done[e] = 0;
  }
  for (int64_t i = tid; i < NK; i += EVAL_BLOCK) {
    s.returns[i] = 0.f;
    s.lengths[i] = 0;
  }
  if (tid == 0) {
    s.words->remaining = NK;
    s.words->steps = 0;
  }
}

// One workgroup: a thread meets the same envs at every call, each env is touched by one thread, and the
// episodes still owed are an integer sum (per-thread partials, then the LDS tree), so no atomics and
// no float reduction.
__global__ __launch_bounds__(EVAL_BLOCK) void eval_step_kernel(EvalStepArgs p) {
  __shared__ long long red[EVAL_BLOCK];
  const int tid = threadIdx.x;
  long long owed = 0;
  for (int e = tid; e < p.s.N; e += EVAL_BLOCK) owed += eval_step_env(p, e);
  red[tid] = owed;
  eval_block_sum(red, tid);
  if (tid == 0) {
    p.s.words->remaining = red[0];
    p.s.words->steps += 1;
  }
}

// The partial of one of the 256 lanes of the summary's reduction, and how two are combined
struct EvalPart {
  int64_t episodes, length_sum;
  double sum, sumsq;
  float mn, mx;
};

__host__ __device__ inline EvalPart eval_part_zero() { return {0, 0, 0.0, 0.0, 0.f, 0.f}; }

__host__ __device__ inline void eval_part_add(EvalPart &a, float ret, int64_t len) {
#pragma clang fp contract(off)
  const double x = (double)ret;
  const double sq = x * x;  // rounded to double before it is added (exact: 24-bit operands)
  a.mn = a.episodes == 0 ? ret : (ret < a.mn ? ret : a.mn);
  a.mx = a.episodes == 0 ? ret : (ret > a.mx ? ret : a.mx);
  a.episodes += 1;
  a.length_sum += len;
  a.sum = a.sum + x;
  a.sumsq = a.sumsq + sq;
}

// a ⊕= b: an empty side contributes nothing to min / max
__host__ __device__ inline void eval_part_merge(EvalPart &a, const EvalPart &b) {
#pragma clang fp contract(off)
  if (b.episodes != 0) {
    a.mn = a.episodes == 0 ? b.mn : (b.mn < a.mn ? b.mn : a.mn);
    a.mx = a.episodes == 0 ? b.mx : (b.mx > a.mx ? b.mx : a.mx);
  }
  a.episodes += b.episodes;
  a.length_sum += b.length_sum;
  a.sum = a.sum + b.sum;
  a.sumsq = a.sumsq + b.sumsq;
}

// Lane j's partial: the finished entries i = j, j + 256, ... in ascending order
__host__ __device__ inline EvalPart eval_lane_part(const mt_eval_state &s, int j) {
  EvalPart a = eval_part_zero();
  const int64_t NK = (int64_t)s.N * s.K;
  for (int64_t i = j; i < NK; i += EVAL_BLOCK) {
    const int64_t e = i / s.K, k = i - e * s.K;
    if (k < (int64_t)s.done[e]) eval_part_add(a, s.returns[i], s.lengths[i]);
  }
  return a;
}

__host__ __device__ inline void eval_write_summary(mt_eval_summary *out, const EvalPart &a, int64_t unfinished) {
  out->episodes = a.episodes;
  out->unfinished = unfinished;
  out->length_sum = a.length_sum;
  out->sum = a.sum;
  out->sumsq = a.sumsq;
  out->min = a.mn;
  out->max = a.mx;
  out->pad[0] = out->pad[1] = 0;
}

__global__ __launch_bounds__(EVAL_BLOCK) void eval_summarize_kernel(mt_eval_state s, mt_eval_summary *out) {
  __shared__ EvalPart part[EVAL_BLOCK];
  const int tid = threadIdx.x;
  part[tid] = eval_lane_part(s, tid);
  __syncthreads();
  for (int h = EVAL_BLOCK / 2; h > 0; h >>= 1) {
    if (tid < h) eval_part_merge(part[tid], part[tid + h]);
    __syncthreads();
  }
  if (tid == 0) eval_write_summary(out, part[0], s.words->remaining);
}

static int eval_check(const mt_eval_state *s, const char *who) {
  MT_CHECK_ARG(s != nullptr, "%s: null state", who);
  MT_CHECK_ARG(s->ret_acc && s->len_acc && s->done && s->returns && s->lengths && s->words,
               "%s: null pointer in the eval state", who);
  MT_CHECK_ARG(s->N >= 1 && s->K >= 1, "%s: N and K must be >= 1", who);
  MT_CHECK_ARG((int64_t)s->N * s->K <= (int64_t)1 << 30, "%s: N * K too large", who);
  MT_CHECK_ARG((((uintptr_t)s->len_acc | (uintptr_t)s->lengths | (uintptr_t)s->words) & 7) == 0,
               "%s: misaligned buffer", who);
  MT_CHECK_ARG((((uintptr_t)s->ret_acc | (uintptr_t)s->done | (uintptr_t)s->returns) & 3) == 0,
               "%s: misaligned buffer", who);
  return MT_OK;
}

static int eval_step_check(const EvalStepArgs &p, const char *who) {
  MT_CHECK_ARG(p.r_idx && p.reward && p.over && p.tab_rep, "%s: null argument", who);
  MT_CHECK_ARG(p.R >= 1, "%s: R must be >= 1", who);
  return MT_OK;
}

static int eval_summary_check(const mt_eval_summary *out, const char *who) {
  MT_CHECK_ARG(out != nullptr, "%s: null summary", who);
  MT_CHECK_ARG(((uintptr_t)out & 7) == 0, "%s: misaligned summary", who);
  return MT_OK;
}

}  // namespace mt

using namespace mt;

extern "C" int mt_eval_reset(const mt_eval_state *state, mt_stream_t stream) {
  if (int rc = eval_check(state, "mt_eval_reset")) return rc;
  hipLaunchKernelGGL(eval_reset_kernel, dim3(1), dim3(EVAL_BLOCK), 0, (hipStream_t)stream, *state);
  MT_LAUNCHED();
  return MT_OK;
}

extern "C" int mt_eval_step(const mt_eval_state *state, const int32_t *r_idx, const float *reward, const float *over,
                            const int32_t *tab_rep, int R, mt_stream_t stream) {
  if (int rc = eval_check(state, "mt_eval_step")) return rc;
  const EvalStepArgs p = {*state, r_idx, reward, over, tab_rep, R};
  if (int rc = eval_step_check(p, "mt_eval_step")) return rc;
  hipLaunchKernelGGL(eval_step_kernel, dim3(1), dim3(EVAL_BLOCK), 0, (hipStream_t)stream, p);
  MT_LAUNCHED();
  return MT_OK;
}

extern "C" int mt_eval_summarize(const mt_eval_state *state, mt_eval_summary *out, mt_stream_t stream) {
  if (int rc = eval_check(state, "mt_eval_summarize")) return rc;
  if (int rc = eval_summary_check(out, "mt_eval_summarize")) return rc;
  hipLaunchKernelGGL(eval_summarize_kernel, dim3(1), dim3(EVAL_BLOCK), 0, (hipStream_t)stream, *state, out);
  MT_LAUNCHED();
  return MT_OK;
}

extern "C" int mt_eval_reset_host(const mt_eval_state *state) {
  if (int rc = eval_check(state, "mt_eval_reset_host")) return rc;
  const mt_eval_state &s = *state;
  const int64_t NK = (int64_t)s.N * s.K;
  for (int e = 0; e < s.N; ++e) {
    s.ret_acc[e] = 0.f;
    s.len_acc[e] = 0;
    s.done[e] = 0;
  }
  for (int64_t i = 0; i < NK; ++i) {
    s.returns[i] = 0.f;
    s.lengths[i] = 0;
  }
  s.words->remaining = NK;
  s.words->steps = 0;
  return MT_OK;
}

extern "C" int mt_eval_step_host(const mt_eval_state *state, const int32_t *r_idx, const float *reward,
                                 const float *over, const int32_t *tab_rep, int R) {
  if (int rc = eval_check(state, "mt_eval_step_host")) return rc;
  const EvalStepArgs p = {*state, r_idx, reward, over, tab_rep, R};
  if (int rc = eval_step_check(p, "mt_eval_step_host")) return rc;
  int64_t owed = 0;
  for (int e = 0; e < p.s.N; ++e) owed += eval_step_env(p, e);
  p.s.words->remaining = owed;
  p.s.words->steps += 1;
  return MT_OK;
}

extern "C" int mt_eval_summarize_host(const mt_eval_state *state, mt_eval_summary *out) {
  if (int rc = eval_check(state, "mt_eval_summarize_host")) return rc;
  if (int rc = eval_summary_check(out, "mt_eval_summarize_host")) return rc;
  static thread_local EvalPart part[EVAL_BLOCK];
  for (int j = 0; j < EVAL_BLOCK; ++j) part[j] = eval_lane_part(*state, j);
  for (int h = EVAL_BLOCK / 2; h > 0; h >>= 1)
    for (int j = 0; j < h; ++j) eval_part_merge(part[j], part[j + h]);
  eval_write_summary(out, part[0], state->words->remaining);
  return MT_OK;
}
