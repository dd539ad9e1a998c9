// Tetris, the third device-resident environment (include/manette_hip.h, "Tetris"; the rule: tetris.h).
// bricks_kernel's contract and launch shape: one kernel per macro-step runs the game logic of every env,
// renders its pushed frames and writes the next stacked state straight into the rollout's state ring.
#include "tetris.h"
#include "device_game.h"

namespace mt {
namespace {

// One workgroup per env. The board is 22 words indexed by run-time rows, and a trace of four snapshots is
// 96 words: far past what scalar registers hold, and a private array would become scratch. So the env's
// board and its trace live in LDS (88 + 396 bytes), the state's scalar fields in registers: thread 0 reads
// the state once, plays the macro-step (at most tab_rep[r] + 1 nexts and a new game's 34 acts, each a handful
// of row tests) through the rule's own functions, and is the one writer of the state and of the per-env
// outputs. One barrier hands the
// trace to the render-and-stack pass over 16-byte pieces of the env's NHWC state, as bricks_kernel's; a
// piece whose cell rows are outside the live mask (rows holding a board cell, the falling piece or the
// next piece in some pushed snapshot) is prev shifted plus the background grid, with no snapshot read.
// prev is not read when all four positions are replaced. RESET: a new game (mt_tetris_reset).
template <int DEPTH, bool RESET>
__global__ __launch_bounds__(256) void tetris_kernel(mt_tetris_config cfg, uint64_t seed, int env0,
                                                     const int32_t *__restrict__ tab_rep, int R,
                                                     const int32_t *__restrict__ a_idx,
                                                     const int32_t *__restrict__ r_idx, mt_tetris_state *state,
                                                     const uint8_t *__restrict__ prev, uint8_t *__restrict__ out,
                                                     uint8_t *__restrict__ frames_out,
                                                     int32_t *__restrict__ push_count_out,
                                                     float *__restrict__ reward_out, float *__restrict__ over_out,
                                                     float *__restrict__ rm_out, int t, int T) {
  __shared__ uint32_t board[kTetrisRows];
  __shared__ TetrisTrace tr;
  const int e = blockIdx.x, E = gridDim.x;
  if (threadIdx.x == 0) {
    const uint64_t genv = (uint64_t)(env0 + e);
    TetrisVars s;
    if constexpr (RESET) {
      tetris_reset(cfg, seed, genv, s, board, tr);
    } else {
      s = tetris_vars(state[e]);
      for (int y = 0; y < kTetrisRows; ++y) board[y] = tetris_board_word(state[e].board[y]);
      int a = a_idx[e], r = r_idx[e];
      a = clamp_index(a, 5);  // (Tetris::kActions)
      r = clamp_index(r, R);
      const int rep = clamp_index(tab_rep[r], 256);
      int reward = 0;
      bool over = false;
      tetris_macro_step(cfg, seed, genv, s, board, a, rep + 1, tr, &reward, &over);
      write_step_outputs(e, E, reward, over, tr.count, push_count_out, reward_out, over_out, rm_out, t, T);
    }
    tetris_store_vars(state[e], s);
    for (int y = 0; y < kTetrisRows; ++y) state[e].board[y] = board[y];
  }
  __syncthreads();  // the trace is complete
  constexpr int N16 = 84 * 84 * DEPTH / 4;  // 16-byte pieces of one env's state (4 words each)
  const size_t base = (size_t)e * N16;
  const u32x4 *pv = reinterpret_cast<const u32x4 *>(prev) + base;
  u32x4 *po = reinterpret_cast<u32x4 *>(out) + base;
  const bool shift = tr.count < 4;  // workgroup-uniform
  for (int i = threadIdx.x; i < N16; i += 256) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (shift) v = pv[i];
    // (the piece's words lie in the pixel rows of its first and last word)
    const bool live = tetris_row_live(tr, (4 * i / DEPTH) / 84) || tetris_row_live(tr, ((4 * i + 3) / DEPTH) / 84);
    if (live) {
      v.x = tetris_word<DEPTH>(4 * i, v.x, tr, true);
      v.y = tetris_word<DEPTH>(4 * i + 1, v.y, tr, true);
      v.z = tetris_word<DEPTH>(4 * i + 2, v.z, tr, true);
      v.w = tetris_word<DEPTH>(4 * i + 3, v.w, tr, true);
    } else {
      v.x = tetris_word<DEPTH>(4 * i, v.x, tr, false);
      v.y = tetris_word<DEPTH>(4 * i + 1, v.y, tr, false);
      v.z = tetris_word<DEPTH>(4 * i + 2, v.z, tr, false);
      v.w = tetris_word<DEPTH>(4 * i + 3, v.w, tr, false);
    }
    po[i] = v;
  }
  if constexpr (!RESET) {
    if (frames_out) {  // the pushes' frames themselves, [84][84][DEPTH] each
      constexpr int F16 = 84 * 84 * DEPTH / 16;
      u32x4 *fo = reinterpret_cast<u32x4 *>(frames_out) + (size_t)4 * e * F16;
      const int n = tr.count, first = tr.pushes - n;
      for (int j = 0; j < n; ++j) {
        const uint32_t *sn = tr.snap[(first + j) & 3];
        for (int q = threadIdx.x; q < F16; q += 256)  // (sn captured by value: the pointer stays in registers)
          fo[(size_t)j * F16 + q] = frame_piece<DEPTH>(q, [sn](int x, int y, int ch) {
            return tetris_shade<DEPTH>(tetris_cell(sn, tetris_cell_col(x), tetris_cell_row(y)), ch);
          });
      }
    }
  }
}

// What device_game.h needs of Tetris. A host state record is played as the kernel plays it: the scalar fields
// as TetrisVars, the board words normalised in place.
struct Tetris {
  static constexpr const char *name = "tetris";
  typedef mt_tetris_config Config;
  typedef mt_tetris_state State;
  typedef TetrisTrace Trace;
  static constexpr int kActions = 5;
  static constexpr const char *config_rule = "max_nexts and speed must be >= 1 and max_start_wait in [0, 30]";
  static bool config_ok(const Config &cfg) {
    return cfg.max_nexts >= 1 && cfg.speed >= 1 && cfg.max_start_wait >= 0 && cfg.max_start_wait <= 30;
  }
  static void new_game(const Config &cfg, uint64_t seed, uint64_t genv, State &st, Trace &tr) {
    TetrisVars s = {};
    tetris_reset(cfg, seed, genv, s, st.board, tr);
    tetris_store_vars(st, s);
  }
  static void macro_step(const Config &cfg, uint64_t seed, uint64_t genv, State &st, int a, int n, Trace &tr,
                         int *reward, bool *over) {
    TetrisVars s = tetris_vars(st);
    for (int y = 0; y < kTetrisRows; ++y) st.board[y] = tetris_board_word(st.board[y]);
    tetris_macro_step(cfg, seed, genv, s, st.board, a, n, tr, reward, over);
    tetris_store_vars(st, s);
  }
  // (every word on the exact path, so the kernel's background shortcut is checked against it)
  template <int DEPTH>
  static uint32_t word(int w, uint32_t prev_word, const Trace &tr) {
    return tetris_word<DEPTH>(w, prev_word, tr, true);
  }
  static const uint32_t *push(const Trace &tr, int j) { return tr.snap[(tr.pushes - tr.count + j) & 3]; }
  template <int DEPTH>
  static uint32_t value(int x, int y, int ch, const uint32_t *sn) {
    return tetris_shade<DEPTH>(tetris_cell(sn, tetris_cell_col(x), tetris_cell_row(y)), ch);
  }
  static GameKernel<Tetris> kernel(int depth, bool reset) {
    return reset ? (depth == 1 ? tetris_kernel<1, true> : tetris_kernel<3, true>)
                 : (depth == 1 ? tetris_kernel<1, false> : tetris_kernel<3, false>);
  }
};

}  // namespace
}  // namespace mt

using namespace mt;

extern "C" int mt_tetris_reset(const mt_tetris_config *cfg, uint64_t seed, int env0, int E, int depth,
                               mt_tetris_state *state, uint8_t *out_state0, mt_stream_t stream) {
  return game_reset<Tetris>(cfg, seed, env0, E, depth, state, out_state0, stream);
}

extern "C" int mt_tetris_step(const mt_tetris_config *cfg, uint64_t seed, int env0, int E, int depth,
                              const int32_t *tab_rep, int R, const int32_t *a_idx, const int32_t *r_idx,
                              mt_tetris_state *state, const uint8_t *prev, uint8_t *out, uint8_t *frames_out,
                              int32_t *push_count_out, float *reward_out, float *over_out, float *rm_out, int t, int T,
                              mt_stream_t stream) {
  return game_step<Tetris>(cfg, seed, env0, E, depth, tab_rep, R, a_idx, r_idx, state, prev, out, frames_out,
                           push_count_out, reward_out, over_out, rm_out, t, T, stream);
}

extern "C" int mt_tetris_reset_host(const mt_tetris_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                                    mt_tetris_state *state, uint8_t *out_state0) {
  return game_reset_host<Tetris>(cfg, seed, global_env, depth, state, out_state0);
}

extern "C" int mt_tetris_step_host(const mt_tetris_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                                   const int32_t *tab_rep, int R, int a, int r, mt_tetris_state *state,
                                   const uint8_t *prev, uint8_t *out, uint8_t *frames_out, int32_t *push_count_out,
                                   float *reward_out, float *over_out) {
  return game_step_host<Tetris>(cfg, seed, global_env, depth, tab_rep, R, a, r, state, prev, out, frames_out,
                                push_count_out, reward_out, over_out);
}
