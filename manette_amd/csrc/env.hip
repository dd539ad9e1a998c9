// Catch, the device-resident environment (include/manette_hip.h, "Catch"; the rule: common.h).
// One kernel per macro-step: the game logic of every env, the renders of its pushed frames and the
// next stacked state, written straight into the rollout's state ring. No staging, no host thread.
#include "common.h"

namespace mt {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }

// An 84-bit mask (rows of the field) in two words; bits (<= 12 wide) are set from `start` <= 80.
struct Mask84 {
  uint64_t lo, hi;
};
__device__ __forceinline__ void mask_or(Mask84 &m, int start, uint64_t bits) {
  if (start < 64) {
    m.lo |= bits << start;
    if (start > 0) m.hi |= bits >> (64 - start);
  } else {
    m.hi |= bits << (start - 64);
  }
}
__device__ __forceinline__ bool mask_bit(const Mask84 &m, int i) {
  return ((i < 64 ? m.lo >> i : m.hi >> (i - 64)) & 1ull) != 0;
}

// One workgroup per env. Every wave runs the env's game logic itself: it depends on blockIdx only, so
// it is wave-uniform scalar work (at most 11 x 4 sub-frames, plus a new game's 16) and needs neither
// LDS nor a barrier to hand its result to the render pass. The one barrier orders every wave's read
// of the env's state before thread 0's write of the new one. Then a single render-and-stack pass:
// each thread takes 16-byte pieces of the env's NHWC state (four words = the four stack bytes of four
// (pixel, channel) pairs), shifts prev's words down by the pushes and inserts the new values, each a
// pure function of (x, y, channel, snapshot). prev is not read when all four positions are replaced.
// RESET: a new game from ball_counter = 0 instead of a macro-step (mt_catch_reset).
template <int DEPTH, bool RESET>
__global__ __launch_bounds__(256) void catch_kernel(mt_catch_config cfg, uint64_t seed, int env0,
                                                    const int32_t *__restrict__ tab_rep, int R,
                                                    const int32_t *__restrict__ a_idx,
                                                    const int32_t *__restrict__ r_idx, mt_catch_state *state,
                                                    const uint8_t *__restrict__ prev, uint8_t *__restrict__ out,
                                                    uint8_t *__restrict__ frames_out,
                                                    int32_t *__restrict__ push_count_out,
                                                    float *__restrict__ reward_out, float *__restrict__ over_out,
                                                    float *__restrict__ rm_out, int t, int T) {
  const int e = blockIdx.x, E = gridDim.x;
  const uint64_t genv = (uint64_t)(env0 + e);
  mt_catch_state s = {};
  CatchTrace tr = {};
  int reward = 0;
  bool over = false;
  if constexpr (RESET) {
    catch_new_game(cfg, seed, genv, s, tr);
  } else {
    const mt_catch_state ld = state[e];
    __syncthreads();  // every wave has read the state before thread 0 replaces it
    // (the same value in every lane: moved to scalar registers, so the logic below is scalar work)
    s.paddle_x = sgpr(ld.paddle_x);
    s.ball_x = sgpr(ld.ball_x);
    s.ball_y = sgpr(ld.ball_y);
    s.ball_dx = sgpr(ld.ball_dx);
    s.misses = sgpr(ld.misses);
    s.balls = sgpr(ld.balls);
    s.ball_counter = (uint64_t)(uint32_t)sgpr((int)(uint32_t)ld.ball_counter) |
                     ((uint64_t)(uint32_t)sgpr((int)(uint32_t)(ld.ball_counter >> 32)) << 32);
    int a = sgpr(a_idx[e]), r = sgpr(r_idx[e]);
    a = a < 0 ? 0 : (a > 2 ? 2 : a);
    r = r < 0 ? 0 : (r > R - 1 ? R - 1 : r);
    int rep = sgpr(tab_rep[r]);
    rep = rep < 0 ? 0 : (rep > 255 ? 255 : rep);
    catch_macro_step(cfg, seed, genv, s, a, rep + 1, tr, &reward, &over);
  }
  if (threadIdx.x == 0) {
    state[e] = s;
    if constexpr (!RESET) {
      const float rw = (float)reward;
      reward_out[e] = rw;
      over_out[e] = over ? 1.f : 0.f;
      rm_out[(size_t)t * E + e] = rw > 1.f ? 1.f : (rw < -1.f ? -1.f : rw);
      rm_out[((size_t)T + t) * E + e] = over ? 0.f : 1.f;
      if (push_count_out) push_count_out[e] = tr.count;
    }
  }
  constexpr int N16 = 84 * 84 * DEPTH / 4;  // 16-byte pieces of one env's state (4 words each)
  const size_t base = (size_t)e * N16;
  const u32x4 *pv = reinterpret_cast<const u32x4 *>(prev) + base;
  u32x4 *po = reinterpret_cast<u32x4 *>(out) + base;
  const bool shift = tr.count < 4;  // wave-uniform
  // rows a sprite of any pushed snapshot touches (a scalar 84-bit mask): every other row of the new
  // frames is background, so a piece lying in such rows is prev shifted (or zero) and skips the renders.
  // (A column mask on top of it measured slower: a wave covers a whole row or more, so it is live
  // whenever its row is, and the per-word tests are paid by every piece.)
  Mask84 rows = {0, 0};
  mask_or(rows, 79, 7);  // the paddle's rows 79..81
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < tr.count) {
      const uint64_t pair = catch_trace_push(tr, j);
      mask_or(rows, (int)((pair >> 16) & 0xffu), 0xf);  // the ball's 4 rows from ball_y, both snapshots
      mask_or(rows, (int)((pair >> 48) & 0xffu), 0xf);
    }
  }
  const int sh = 8 * tr.count;
  for (int i = threadIdx.x; i < N16; i += 256) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (shift) v = pv[i];
    // (the piece's words lie in the rows of its first and last word)
    const bool live = mask_bit(rows, (4 * i / DEPTH) / 84) || mask_bit(rows, ((4 * i + 3) / DEPTH) / 84);
    if (live) {
      v.x = catch_word<DEPTH>(4 * i, v.x, tr);
      v.y = catch_word<DEPTH>(4 * i + 1, v.y, tr);
      v.z = catch_word<DEPTH>(4 * i + 2, v.z, tr);
      v.w = catch_word<DEPTH>(4 * i + 3, v.w, tr);
    } else if (shift) {
      v.x >>= sh;
      v.y >>= sh;
      v.z >>= sh;
      v.w >>= sh;
    }
    po[i] = v;
  }
  if constexpr (!RESET) {
    if (frames_out) {  // the pushes' frames themselves, [84][84][DEPTH] each, 16 bytes per thread and turn
      constexpr int F16 = 84 * 84 * DEPTH / 16;
      for (int i = threadIdx.x; i < tr.count * F16; i += 256) {
        const int j = i / F16, q = i - j * F16;
        const uint64_t pair = catch_trace_push(tr, j);
        u32x4 v;
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          w[k] = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int byte = 16 * q + 4 * k + b, pix = byte / DEPTH, ch = byte - pix * DEPTH;
            const int y = pix / 84, x = pix - y * 84;
            w[k] |= catch_value<DEPTH>(x, y, ch, pair) << (8 * b);
          }
        }
        v.x = w[0];
        v.y = w[1];
        v.z = w[2];
        v.w = w[3];
        reinterpret_cast<u32x4 *>(frames_out)[((size_t)4 * e + j) * F16 + q] = v;
      }
    }
  }
}

static int catch_check(const mt_catch_config *cfg, int depth, const char *who) {
  MT_CHECK_ARG(cfg != nullptr, "%s: null config", who);
  MT_CHECK_ARG(depth == 1 || depth == 3, "%s: depth must be 1 or 3", who);
  MT_CHECK_ARG(cfg->lives >= 1 && cfg->max_balls >= 1, "%s: lives and max_balls must be >= 1", who);
  return MT_OK;
}

// Host render of one env's stacked state / frames from a trace (the kernel's word and byte functions).
template <int DEPTH>
static void host_stack(const CatchTrace &tr, const uint8_t *prev, uint8_t *out) {
  for (int w = 0; w < 84 * 84 * DEPTH; ++w) {
    uint32_t pw = 0;
    if (tr.count < 4) memcpy(&pw, prev + 4 * (size_t)w, 4);
    const uint32_t v = catch_word<DEPTH>(w, pw, tr);
    memcpy(out + 4 * (size_t)w, &v, 4);
  }
}
template <int DEPTH>
static void host_frames(const CatchTrace &tr, uint8_t *frames) {
  for (int j = 0; j < tr.count; ++j) {
    const uint64_t pair = catch_trace_push(tr, j);
    uint8_t *f = frames + (size_t)j * 84 * 84 * DEPTH;
    for (int pix = 0; pix < 84 * 84; ++pix)
      for (int ch = 0; ch < DEPTH; ++ch) f[pix * DEPTH + ch] = (uint8_t)catch_value<DEPTH>(pix % 84, pix / 84, ch, pair);
  }
}

}  // namespace mt

using namespace mt;

extern "C" int mt_catch_reset(const mt_catch_config *cfg, uint64_t seed, int env0, int E, int depth,
                              mt_catch_state *state, uint8_t *out_state0, mt_stream_t stream) {
  if (int rc = catch_check(cfg, depth, "mt_catch_reset")) return rc;
  MT_CHECK_ARG(E >= 1 && env0 >= 0, "mt_catch_reset: E must be >= 1 and env0 >= 0");
  MT_CHECK_ARG(state && out_state0, "mt_catch_reset: null argument");
  MT_CHECK_ARG(((uintptr_t)out_state0 & 15) == 0 && ((uintptr_t)state & 7) == 0, "mt_catch_reset: misaligned buffer");
  if (depth == 1)
    hipLaunchKernelGGL((catch_kernel<1, true>), dim3(E), dim3(256), 0, (hipStream_t)stream, *cfg, seed, env0, nullptr, 1,
                       nullptr, nullptr, state, nullptr, out_state0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1);
  else
    hipLaunchKernelGGL((catch_kernel<3, true>), dim3(E), dim3(256), 0, (hipStream_t)stream, *cfg, seed, env0, nullptr, 1,
                       nullptr, nullptr, state, nullptr, out_state0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1);
  MT_LAUNCHED();
  return MT_OK;
}

extern "C" int mt_catch_step(const mt_catch_config *cfg, uint64_t seed, int env0, int E, int depth,
                             const int32_t *tab_rep, int R, const int32_t *a_idx, const int32_t *r_idx,
                             mt_catch_state *state, const uint8_t *prev, uint8_t *out, uint8_t *frames_out,
                             int32_t *push_count_out, float *reward_out, float *over_out, float *rm_out, int t, int T,
                             mt_stream_t stream) {
  if (int rc = catch_check(cfg, depth, "mt_catch_step")) return rc;
  MT_CHECK_ARG(E >= 1 && env0 >= 0 && R >= 1, "mt_catch_step: E and R must be >= 1 and env0 >= 0");
  MT_CHECK_ARG(T >= 1 && t >= 0 && t < T, "mt_catch_step: t must be in [0, T)");
  MT_CHECK_ARG(tab_rep && a_idx && r_idx && state && prev && out && reward_out && over_out && rm_out,
               "mt_catch_step: null argument");
  MT_CHECK_ARG((frames_out == nullptr) == (push_count_out == nullptr),
               "mt_catch_step: frames_out and push_count_out go together");
  MT_CHECK_ARG(prev != out, "mt_catch_step: out may not alias prev");
  MT_CHECK_ARG((((uintptr_t)prev | (uintptr_t)out | (uintptr_t)frames_out) & 15) == 0 && ((uintptr_t)state & 7) == 0,
               "mt_catch_step: misaligned buffer");
  if (depth == 1)
    hipLaunchKernelGGL((catch_kernel<1, false>), dim3(E), dim3(256), 0, (hipStream_t)stream, *cfg, seed, env0, tab_rep, R,
                       a_idx, r_idx, state, prev, out, frames_out, push_count_out, reward_out, over_out, rm_out, t, T);
  else
    hipLaunchKernelGGL((catch_kernel<3, false>), dim3(E), dim3(256), 0, (hipStream_t)stream, *cfg, seed, env0, tab_rep, R,
                       a_idx, r_idx, state, prev, out, frames_out, push_count_out, reward_out, over_out, rm_out, t, T);
  MT_LAUNCHED();
  return MT_OK;
}

extern "C" int mt_catch_reset_host(const mt_catch_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                                   mt_catch_state *state, uint8_t *out_state0) {
  if (int rc = catch_check(cfg, depth, "mt_catch_reset_host")) return rc;
  MT_CHECK_ARG(state != nullptr, "mt_catch_reset_host: null state");
  mt_catch_state s = {};
  CatchTrace tr = {};
  catch_new_game(*cfg, seed, global_env, s, tr);
  *state = s;
  if (out_state0) {
    if (depth == 1)
      host_stack<1>(tr, nullptr, out_state0);
    else
      host_stack<3>(tr, nullptr, out_state0);
  }
  return MT_OK;
}

extern "C" int mt_catch_step_host(const mt_catch_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                                  const int32_t *tab_rep, int R, int a, int r, mt_catch_state *state,
                                  const uint8_t *prev, uint8_t *out, uint8_t *frames_out, int32_t *push_count_out,
                                  float *reward_out, float *over_out) {
  if (int rc = catch_check(cfg, depth, "mt_catch_step_host")) return rc;
  MT_CHECK_ARG(tab_rep && R >= 1 && state && reward_out && over_out, "mt_catch_step_host: null argument or R < 1");
  MT_CHECK_ARG(!out || (prev && prev != out), "mt_catch_step_host: out needs a prev that it does not alias");
  a = a < 0 ? 0 : (a > 2 ? 2 : a);
  r = r < 0 ? 0 : (r > R - 1 ? R - 1 : r);
  int rep = tab_rep[r];
  rep = rep < 0 ? 0 : (rep > 255 ? 255 : rep);
  mt_catch_state s = *state;
  CatchTrace tr = {};
  int reward;
  bool over;
  catch_macro_step(*cfg, seed, global_env, s, a, rep + 1, tr, &reward, &over);
  *state = s;
  *reward_out = (float)reward;
  *over_out = over ? 1.f : 0.f;
  if (push_count_out) *push_count_out = tr.count;
  if (out) {
    if (depth == 1)
      host_stack<1>(tr, prev, out);
    else
      host_stack<3>(tr, prev, out);
  }
  if (frames_out) {
    if (depth == 1)
      host_frames<1>(tr, frames_out);
    else
      host_frames<3>(tr, frames_out);
  }
  return MT_OK;
}
