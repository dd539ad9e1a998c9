// The device games' shared layer (include/manette_hip.h: "Catch", "Bricks", "Tetris"). Every game has the
// same four entry points, mt_<game>_reset / _step (one kernel per macro-step) and mt_<game>_reset_host /
// _step_host (the same rule on the host): their argument checks, index clamps, depth dispatch and host
// renders are written here once, over a traits type G that each game defines next to its kernel
// (catch.hip, bricks.hip, tetris.hip) and that supplies nothing but what is the game's own:
//   G::name                        "catch": the messages name the entry point, "mt_catch_step: ..."
//   G::Config, G::State, G::Trace  mt_<game>_config, mt_<game>_state, the pushes of one macro-step
//   G::kActions                    the action count (a is clamped to [0, kActions))
//   G::config_ok(cfg), G::config_rule   the config check and its message
//   G::new_game(cfg, seed, genv, state, tr)                          on a zeroed host state record
//   G::macro_step(cfg, seed, genv, state, a, n, tr, &reward, &over)  on a host state record, in place
//   G::word<DEPTH>(w, prev_word, tr)   32-bit word w of the next stacked state (the kernel's function)
//   G::push(tr, j), G::value<DEPTH>(x, y, ch, push)   push j (oldest first) and a byte of its own frame
//   G::kernel(depth, reset)        the game's four kernel instantiations, all of the type GameKernel<G>
// The kernels stay the games' own; they share the small device helpers at the end of this file.
#pragma once
#include "common.h"

namespace mt {

template <class G>
using GameKernel = void (*)(typename G::Config cfg, uint64_t seed, int env0, const int32_t *tab_rep, int R,
                            const int32_t *a_idx, const int32_t *r_idx, typename G::State *state, const uint8_t *prev,
                            uint8_t *out, uint8_t *frames_out, int32_t *push_count_out, float *reward_out,
                            float *over_out, float *rm_out, int t, int T);

// v clamped to [0, n): an action index against the game's count, a repetition index against R, a table entry
// against 256 (a macro-step plays at most 256 nexts)
__host__ __device__ __forceinline__ int clamp_index(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// The checks every entry point starts with; fn: "reset", "step", "reset_host" or "step_host".
template <class G>
int game_check(const typename G::Config *cfg, int depth, const char *fn) {
  MT_CHECK_ARG(cfg != nullptr, "mt_%s_%s: null config", G::name, fn);
  MT_CHECK_ARG(depth == 1 || depth == 3, "mt_%s_%s: depth must be 1 or 3", G::name, fn);
  MT_CHECK_ARG(G::config_ok(*cfg), "mt_%s_%s: %s", G::name, fn, G::config_rule);
  return MT_OK;
}

// Host render of one env's stacked state / frames from a trace (the kernel's word and byte functions).
template <class G, int DEPTH>
void host_stack(const typename G::Trace &tr, const uint8_t *prev, uint8_t *out) {
  for (int w = 0; w < 84 * 84 * DEPTH; ++w) {
    uint32_t pw = 0;
    if (tr.count < 4) memcpy(&pw, prev + 4 * (size_t)w, 4);
    const uint32_t v = G::template word<DEPTH>(w, pw, tr);
    memcpy(out + 4 * (size_t)w, &v, 4);
  }
}
template <class G, int DEPTH>
void host_frames(const typename G::Trace &tr, uint8_t *frames) {
  for (int j = 0; j < tr.count; ++j) {
    const auto push = G::push(tr, j);
    uint8_t *f = frames + (size_t)j * 84 * 84 * DEPTH;
    for (int pix = 0; pix < 84 * 84; ++pix)
      for (int ch = 0; ch < DEPTH; ++ch)
        f[pix * DEPTH + ch] = (uint8_t)G::template value<DEPTH>(pix % 84, pix / 84, ch, push);
  }
}
template <class G>
void host_stack(int depth, const typename G::Trace &tr, const uint8_t *prev, uint8_t *out) {
  if (depth == 1)
    host_stack<G, 1>(tr, prev, out);
  else
    host_stack<G, 3>(tr, prev, out);
}

template <class G>
int game_reset(const typename G::Config *cfg, uint64_t seed, int env0, int E, int depth, typename G::State *state,
               uint8_t *out_state0, mt_stream_t stream) {
  if (int rc = game_check<G>(cfg, depth, "reset")) return rc;
  MT_CHECK_ARG(E >= 1 && env0 >= 0, "mt_%s_reset: E must be >= 1 and env0 >= 0", G::name);
  MT_CHECK_ARG(state && out_state0, "mt_%s_reset: null argument", G::name);
  MT_CHECK_ARG(((uintptr_t)out_state0 & 15) == 0 && ((uintptr_t)state & 7) == 0, "mt_%s_reset: misaligned buffer",
               G::name);
  hipLaunchKernelGGL(G::kernel(depth, true), dim3(E), dim3(256), 0, (hipStream_t)stream, *cfg, seed, env0, nullptr, 1,
                     nullptr, nullptr, state, nullptr, out_state0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1);
  MT_LAUNCHED();
  return MT_OK;
}

template <class G>
int game_step(const typename G::Config *cfg, uint64_t seed, int env0, int E, int depth, const int32_t *tab_rep, int R,
              const int32_t *a_idx, const int32_t *r_idx, typename G::State *state, const uint8_t *prev, uint8_t *out,
              uint8_t *frames_out, int32_t *push_count_out, float *reward_out, float *over_out, float *rm_out, int t,
              int T, mt_stream_t stream) {
  if (int rc = game_check<G>(cfg, depth, "step")) return rc;
  MT_CHECK_ARG(E >= 1 && env0 >= 0 && R >= 1, "mt_%s_step: E and R must be >= 1 and env0 >= 0", G::name);
  MT_CHECK_ARG(T >= 1 && t >= 0 && t < T, "mt_%s_step: t must be in [0, T)", G::name);
  MT_CHECK_ARG(tab_rep && a_idx && r_idx && state && prev && out && reward_out && over_out && rm_out,
               "mt_%s_step: null argument", G::name);
  MT_CHECK_ARG((frames_out == nullptr) == (push_count_out == nullptr),
               "mt_%s_step: frames_out and push_count_out go together", G::name);
  MT_CHECK_ARG(prev != out, "mt_%s_step: out may not alias prev", G::name);
  MT_CHECK_ARG((((uintptr_t)prev | (uintptr_t)out | (uintptr_t)frames_out) & 15) == 0 && ((uintptr_t)state & 7) == 0,
               "mt_%s_step: misaligned buffer", G::name);
  hipLaunchKernelGGL(G::kernel(depth, false), dim3(E), dim3(256), 0, (hipStream_t)stream, *cfg, seed, env0, tab_rep, R,
                     a_idx, r_idx, state, prev, out, frames_out, push_count_out, reward_out, over_out, rm_out, t, T);
  MT_LAUNCHED();
  return MT_OK;
}

template <class G>
int game_reset_host(const typename G::Config *cfg, uint64_t seed, uint64_t global_env, int depth,
                    typename G::State *state, uint8_t *out_state0) {
  if (int rc = game_check<G>(cfg, depth, "reset_host")) return rc;
  MT_CHECK_ARG(state != nullptr, "mt_%s_reset_host: null state", G::name);
  typename G::State s = {};
  typename G::Trace tr = {};
  G::new_game(*cfg, seed, global_env, s, tr);
  *state = s;
  if (out_state0) host_stack<G>(depth, tr, nullptr, out_state0);
  return MT_OK;
}

template <class G>
int game_step_host(const typename G::Config *cfg, uint64_t seed, uint64_t global_env, int depth,
                   const int32_t *tab_rep, int R, int a, int r, typename G::State *state, const uint8_t *prev,
                   uint8_t *out, uint8_t *frames_out, int32_t *push_count_out, float *reward_out, float *over_out) {
  if (int rc = game_check<G>(cfg, depth, "step_host")) return rc;
  MT_CHECK_ARG(tab_rep && R >= 1 && state && reward_out && over_out, "mt_%s_step_host: null argument or R < 1",
               G::name);
  MT_CHECK_ARG(!out || (prev && prev != out), "mt_%s_step_host: out needs a prev that it does not alias", G::name);
  a = clamp_index(a, G::kActions);
  r = clamp_index(r, R);
  const int rep = clamp_index(tab_rep[r], 256);
  typename G::State s = *state;
  typename G::Trace tr = {};
  int reward;
  bool over;
  G::macro_step(*cfg, seed, global_env, s, a, rep + 1, tr, &reward, &over);
  *state = s;
  *reward_out = (float)reward;
  *over_out = over ? 1.f : 0.f;
  if (push_count_out) *push_count_out = tr.count;
  if (out) host_stack<G>(depth, tr, prev, out);
  if (frames_out) {
    if (depth == 1)
      host_frames<G, 1>(tr, frames_out);
    else
      host_frames<G, 3>(tr, frames_out);
  }
  return MT_OK;
}

// ---- device helpers of the three kernels ----
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// A wave-uniform value moved to scalar registers, so the logic on it is scalar work.
__device__ __forceinline__ int sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t sgpr_u(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t sgpr_u64(uint64_t v) {
  return (uint64_t)sgpr_u((uint32_t)v) | ((uint64_t)sgpr_u((uint32_t)(v >> 32)) << 32);
}

// The rows of the field (an 84-bit mask in two words) that any sprite of a pushed snapshot touches.
struct Rows84 {
  uint64_t lo, hi;
};
// bits (<= 12 wide) are set from `start` <= 81
__device__ __forceinline__ void rows_or(Rows84 &m, int start, uint64_t bits) {
  if (start < 64) {
    m.lo |= bits << start;
    if (start > 0) m.hi |= bits >> (64 - start);
  } else {
    m.hi |= bits << (start - 64);
  }
}
__device__ __forceinline__ bool rows_bit(const Rows84 &m, int i) {
  return ((i < 64 ? m.lo >> (i & 63) : m.hi >> ((i - 64) & 63)) & 1ull) != 0;
}

// The 16-byte piece q of a frame [84][84][DEPTH] whose bytes are value(x, y, ch).
template <int DEPTH, class F>
__device__ __forceinline__ u32x4 frame_piece(int q, F value) {
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w[k] = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int byte = 16 * q + 4 * k + b, pix = byte / DEPTH, ch = byte - pix * DEPTH;
      const int y = pix / 84, x = pix - y * 84;
      w[k] |= value(x, y, ch) << (8 * b);
    }
  }
  u32x4 v;
  v.x = w[0];
  v.y = w[1];
  v.z = w[2];
  v.w = w[3];
  return v;
}

// What one thread of an env's workgroup writes after a macro-step: the reward, the over flag, row t of
// rm [2][T][E] (the clipped reward, the episode mask) and the push count.
__device__ __forceinline__ void write_step_outputs(int e, int E, int reward, bool over, int count,
                                                   int32_t *__restrict__ push_count_out,
                                                   float *__restrict__ reward_out, float *__restrict__ over_out,
                                                   float *__restrict__ rm_out, int t, int T) {
  const float rw = (float)reward;
  reward_out[e] = rw;
  over_out[e] = over ? 1.f : 0.f;
  rm_out[(size_t)t * E + e] = rw > 1.f ? 1.f : (rw < -1.f ? -1.f : rw);
  rm_out[((size_t)T + t) * E + e] = over ? 0.f : 1.f;
  if (push_count_out) push_count_out[e] = count;
}

}  // namespace mt
