// Bricks, the second device-resident environment (include/manette_hip.h, "Bricks"; the rule: bricks.h).
// catch_kernel's shape: one kernel per macro-step runs the game logic of every env, renders its pushed
// frames and writes the next stacked state straight into the rollout's state ring.
#include "bricks.h"
#include "device_game.h"

namespace mt {
namespace {

__device__ __forceinline__ void rows_of_snap(Rows84 &m, const BricksSnap &sn) {
  rows_or(m, (int)((sn.pos >> 16) & 0xffu), 3);  // the ball's 2 rows from ball_y <= 79
#pragma unroll
  for (int r = 0; r < 6; ++r)  // a brick row that still holds a brick: its 3 pixel rows 16 + 3r .. (all below 64)
    if (bricks_row_bits(sn.lo, sn.hi, r) != 0) m.lo |= 7ull << (16 + 3 * r);
}
__device__ __forceinline__ void rows_of_push(Rows84 &m, const BricksPush &p) {
  rows_of_snap(m, p.a);
  rows_of_snap(m, p.b);
}

template <int DEPTH>
__device__ __forceinline__ void write_frame(u32x4 *dst, const BricksPush &p) {
  for (int q = threadIdx.x; q < 84 * 84 * DEPTH / 16; q += 256)
    dst[q] = frame_piece<DEPTH>(q, [&](int x, int y, int ch) {
      return bricks_value<DEPTH>(x, y, ch, bricks_pixel<DEPTH>(x, y, ch), p);
    });
}

// One workgroup per env. Every wave runs the env's game logic itself: it depends on blockIdx only, so
// it is wave-uniform scalar work (at most 11 x 4 sub-frames) on a state moved to scalar registers, and
// needs neither LDS nor a barrier to hand its result (the trace: 4 pushes x 2 snapshots x (positions +
// 84-bit bitmap) = 32 scalar words) to the render pass. The one barrier orders every wave's read of the
// env's state before thread 0's write of the new one. Then a single render-and-stack pass over 16-byte
// pieces of the env's NHWC state, as catch_kernel's; a piece outside the live rows (rows of the brick band
// that hold a brick in some pushed snapshot, the balls' rows, the paddle's rows) is prev shifted or zero.
// prev is not read when all four positions are replaced. RESET: a new game (mt_bricks_reset).
template <int DEPTH, bool RESET>
__global__ __launch_bounds__(256) void bricks_kernel(mt_bricks_config cfg, uint64_t seed, int env0,
                                                     const int32_t *__restrict__ tab_rep, int R,
                                                     const int32_t *__restrict__ a_idx,
                                                     const int32_t *__restrict__ r_idx, mt_bricks_state *state,
                                                     const uint8_t *__restrict__ prev, uint8_t *__restrict__ out,
                                                     uint8_t *__restrict__ frames_out,
                                                     int32_t *__restrict__ push_count_out,
                                                     float *__restrict__ reward_out, float *__restrict__ over_out,
                                                     float *__restrict__ rm_out, int t, int T) {
  const int e = blockIdx.x, E = gridDim.x;
  const uint64_t genv = (uint64_t)(env0 + e);
  mt_bricks_state s = {};
  BricksTrace tr = {};
  int reward = 0;
  bool over = false;
  if constexpr (RESET) {
    bricks_new_game(cfg, s, tr);  // (serve_counter = 0)
  } else {
    const mt_bricks_state ld = state[e];
    __syncthreads();  // every wave has read the state before thread 0 replaces it
    s.paddle_x = sgpr(ld.paddle_x);
    s.ball_x = sgpr(ld.ball_x);
    s.ball_y = sgpr(ld.ball_y);
    s.ball_dx = sgpr(ld.ball_dx);
    s.ball_dy = sgpr(ld.ball_dy);
    s.lives = sgpr(ld.lives);
    s.nexts = sgpr(ld.nexts);
    s.wait = sgpr(ld.wait);
    s.bricks_lo = sgpr_u64(ld.bricks_lo);
    s.bricks_hi = sgpr_u(ld.bricks_hi) & kBricksFullHi;
    s.reserved = 0;
    s.serve_counter = sgpr_u64(ld.serve_counter);
    int a = sgpr(a_idx[e]), r = sgpr(r_idx[e]);
    a = clamp_index(a, 4);  // (Bricks::kActions)
    r = clamp_index(r, R);
    const int rep = clamp_index(sgpr(tab_rep[r]), 256);
    bricks_macro_step(cfg, seed, genv, s, a, rep + 1, tr, &reward, &over);
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
  Rows84 rows = {0, 0};
  rows_or(rows, 79, 7);  // the paddle's rows 79..81
  if (tr.count >= 4) rows_of_push(rows, tr.q0);
  if (tr.count >= 3) rows_of_push(rows, tr.q1);
  if (tr.count >= 2) rows_of_push(rows, tr.q2);
  if (tr.count >= 1) rows_of_push(rows, tr.q3);
  const int sh = 8 * tr.count;
  for (int i = threadIdx.x; i < N16; i += 256) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (shift) v = pv[i];
    // (the piece's words lie in the rows of its first and last word)
    const bool live = rows_bit(rows, (4 * i / DEPTH) / 84) || rows_bit(rows, ((4 * i + 3) / DEPTH) / 84);
    if (live) {
      v.x = bricks_word<DEPTH>(4 * i, v.x, tr);
      v.y = bricks_word<DEPTH>(4 * i + 1, v.y, tr);
      v.z = bricks_word<DEPTH>(4 * i + 2, v.z, tr);
      v.w = bricks_word<DEPTH>(4 * i + 3, v.w, tr);
    } else if (shift) {
      v.x >>= sh;
      v.y >>= sh;
      v.z >>= sh;
      v.w >>= sh;
    }
    po[i] = v;
  }
  if constexpr (!RESET) {
    if (frames_out) {  // the pushes' frames themselves, [84][84][DEPTH] each; the push is chosen by a scalar
      constexpr int F16 = 84 * 84 * DEPTH / 16;
      u32x4 *fo = reinterpret_cast<u32x4 *>(frames_out) + (size_t)4 * e * F16;
      const int n = tr.count;  // push j is q[4 - n + j]: each named by a constant, so the trace stays in registers
      if (n >= 4) write_frame<DEPTH>(fo, tr.q0);
      if (n >= 3) write_frame<DEPTH>(fo + (size_t)(n - 3) * F16, tr.q1);
      if (n >= 2) write_frame<DEPTH>(fo + (size_t)(n - 2) * F16, tr.q2);
      if (n >= 1) write_frame<DEPTH>(fo + (size_t)(n - 1) * F16, tr.q3);
    }
  }
}

// What device_game.h needs of Bricks.
struct Bricks {
  static constexpr const char *name = "bricks";
  typedef mt_bricks_config Config;
  typedef mt_bricks_state State;
  typedef BricksTrace Trace;
  static constexpr int kActions = 4;
  static constexpr const char *config_rule = "lives and max_nexts must be >= 1 and serve_wait >= 0";
  static bool config_ok(const Config &cfg) { return cfg.lives >= 1 && cfg.max_nexts >= 1 && cfg.serve_wait >= 0; }
  // (a new game draws nothing: the first serve hashes seed and genv)
  static void new_game(const Config &cfg, uint64_t, uint64_t, State &s, Trace &tr) { bricks_new_game(cfg, s, tr); }
  static void macro_step(const Config &cfg, uint64_t seed, uint64_t genv, State &s, int a, int n, Trace &tr,
                         int *reward, bool *over) {
    s.bricks_hi &= kBricksFullHi;
    s.reserved = 0;
    bricks_macro_step(cfg, seed, genv, s, a, n, tr, reward, over);
  }
  template <int DEPTH>
  static uint32_t word(int w, uint32_t prev_word, const Trace &tr) {
    return bricks_word<DEPTH>(w, prev_word, tr);
  }
  static const BricksPush *push(const Trace &tr, int j) {
    const BricksPush *q[4] = {&tr.q0, &tr.q1, &tr.q2, &tr.q3};
    return q[4 - tr.count + j];
  }
  template <int DEPTH>
  static uint32_t value(int x, int y, int ch, const BricksPush *p) {
    return bricks_value<DEPTH>(x, y, ch, bricks_pixel<DEPTH>(x, y, ch), *p);
  }
  static GameKernel<Bricks> kernel(int depth, bool reset) {
    return reset ? (depth == 1 ? bricks_kernel<1, true> : bricks_kernel<3, true>)
                 : (depth == 1 ? bricks_kernel<1, false> : bricks_kernel<3, false>);
  }
};

}  // namespace
}  // namespace mt

using namespace mt;

extern "C" int mt_bricks_reset(const mt_bricks_config *cfg, uint64_t seed, int env0, int E, int depth,
                               mt_bricks_state *state, uint8_t *out_state0, mt_stream_t stream) {
  return game_reset<Bricks>(cfg, seed, env0, E, depth, state, out_state0, stream);
}

extern "C" int mt_bricks_step(const mt_bricks_config *cfg, uint64_t seed, int env0, int E, int depth,
                              const int32_t *tab_rep, int R, const int32_t *a_idx, const int32_t *r_idx,
                              mt_bricks_state *state, const uint8_t *prev, uint8_t *out, uint8_t *frames_out,
                              int32_t *push_count_out, float *reward_out, float *over_out, float *rm_out, int t, int T,
                              mt_stream_t stream) {
  return game_step<Bricks>(cfg, seed, env0, E, depth, tab_rep, R, a_idx, r_idx, state, prev, out, frames_out,
                           push_count_out, reward_out, over_out, rm_out, t, T, stream);
}

extern "C" int mt_bricks_reset_host(const mt_bricks_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                                    mt_bricks_state *state, uint8_t *out_state0) {
  return game_reset_host<Bricks>(cfg, seed, global_env, depth, state, out_state0);
}

extern "C" int mt_bricks_step_host(const mt_bricks_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                                   const int32_t *tab_rep, int R, int a, int r, mt_bricks_state *state,
                                   const uint8_t *prev, uint8_t *out, uint8_t *frames_out, int32_t *push_count_out,
                                   float *reward_out, float *over_out) {
  return game_step_host<Bricks>(cfg, seed, global_env, depth, tab_rep, R, a, r, state, prev, out, frames_out,
                                push_count_out, reward_out, over_out);
}
