// Catch, the device-resident environment (include/manette_hip.h, "Catch"; the rule: catch.h).
// One kernel per macro-step: the game logic of every env, the renders of its pushed frames and the
// next stacked state, written straight into the rollout's state ring. No staging, no host thread.
#include "catch.h"
#include "device_game.h"

namespace mt {

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
    s.ball_counter = sgpr_u64(ld.ball_counter);
    int a = sgpr(a_idx[e]), r = sgpr(r_idx[e]);
    a = clamp_index(a, 3);  // (Catch::kActions)
    r = clamp_index(r, R);
    const int rep = clamp_index(sgpr(tab_rep[r]), 256);
    catch_macro_step(cfg, seed, genv, s, a, rep + 1, tr, &reward, &over);
  }
  if (threadIdx.x == 0) {
    state[e] = s;
    if constexpr (!RESET)
      write_step_outputs(e, E, reward, over, tr.count, push_count_out, reward_out, over_out, rm_out, t, T);
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
  Rows84 rows = {0, 0};
  rows_or(rows, 79, 7);  // the paddle's rows 79..81
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < tr.count) {
      const uint64_t pair = catch_trace_push(tr, j);
      rows_or(rows, (int)((pair >> 16) & 0xffu), 0xf);  // the ball's 4 rows from ball_y, both snapshots
      rows_or(rows, (int)((pair >> 48) & 0xffu), 0xf);
    }
  }
  const int sh = 8 * tr.count;
  for (int i = threadIdx.x; i < N16; i += 256) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (shift) v = pv[i];
    // (the piece's words lie in the rows of its first and last word)
    const bool live = rows_bit(rows, (4 * i / DEPTH) / 84) || rows_bit(rows, ((4 * i + 3) / DEPTH) / 84);
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
        // (device_game.h's frame_piece, written out: through it this loop is scheduled differently)
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

// What device_game.h needs of Catch.
struct Catch {
  static constexpr const char *name = "catch";
  typedef mt_catch_config Config;
  typedef mt_catch_state State;
  typedef CatchTrace Trace;
  static constexpr int kActions = 3;
  static constexpr const char *config_rule = "lives and max_balls must be >= 1";
  static bool config_ok(const Config &cfg) { return cfg.lives >= 1 && cfg.max_balls >= 1; }
  static void new_game(const Config &cfg, uint64_t seed, uint64_t genv, State &s, Trace &tr) {
    catch_new_game(cfg, seed, genv, s, tr);
  }
  static void macro_step(const Config &cfg, uint64_t seed, uint64_t genv, State &s, int a, int n, Trace &tr,
                         int *reward, bool *over) {
    catch_macro_step(cfg, seed, genv, s, a, n, tr, reward, over);
  }
  template <int DEPTH>
  static uint32_t word(int w, uint32_t prev_word, const Trace &tr) {
    return catch_word<DEPTH>(w, prev_word, tr);
  }
  static uint64_t push(const Trace &tr, int j) { return catch_trace_push(tr, j); }
  template <int DEPTH>
  static uint32_t value(int x, int y, int ch, uint64_t pair) {
    return catch_value<DEPTH>(x, y, ch, pair);
  }
  static GameKernel<Catch> kernel(int depth, bool reset) {
    return reset ? (depth == 1 ? catch_kernel<1, true> : catch_kernel<3, true>)
                 : (depth == 1 ? catch_kernel<1, false> : catch_kernel<3, false>);
  }
};

}  // namespace mt

using namespace mt;

extern "C" int mt_catch_reset(const mt_catch_config *cfg, uint64_t seed, int env0, int E, int depth,
                              mt_catch_state *state, uint8_t *out_state0, mt_stream_t stream) {
  return game_reset<Catch>(cfg, seed, env0, E, depth, state, out_state0, stream);
}

extern "C" int mt_catch_step(const mt_catch_config *cfg, uint64_t seed, int env0, int E, int depth,
                             const int32_t *tab_rep, int R, const int32_t *a_idx, const int32_t *r_idx,
                             mt_catch_state *state, const uint8_t *prev, uint8_t *out, uint8_t *frames_out,
                             int32_t *push_count_out, float *reward_out, float *over_out, float *rm_out, int t, int T,
                             mt_stream_t stream) {
  return game_step<Catch>(cfg, seed, env0, E, depth, tab_rep, R, a_idx, r_idx, state, prev, out, frames_out,
                          push_count_out, reward_out, over_out, rm_out, t, T, stream);
}

extern "C" int mt_catch_reset_host(const mt_catch_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                                   mt_catch_state *state, uint8_t *out_state0) {
  return game_reset_host<Catch>(cfg, seed, global_env, depth, state, out_state0);
}

extern "C" int mt_catch_step_host(const mt_catch_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                                  const int32_t *tab_rep, int R, int a, int r, mt_catch_state *state,
                                  const uint8_t *prev, uint8_t *out, uint8_t *frames_out, int32_t *push_count_out,
                                  float *reward_out, float *over_out) {
  return game_step_host<Catch>(cfg, seed, global_env, depth, tab_rep, R, a, r, state, prev, out, frames_out,
                               push_count_out, reward_out, over_out);
}
