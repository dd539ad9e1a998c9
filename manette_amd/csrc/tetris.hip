// Tetris, the third device-resident environment (include/manette_hip.h, "Tetris"; the rule: tetris.h).
// bricks_kernel's contract and launch shape: one kernel per macro-step runs the game logic of every env,
// renders its pushed frames and writes the next stacked state straight into the rollout's state ring.
#include "tetris.h"

namespace mt {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The bytes of 16-byte piece q of a snapshot's own frame [84][84][DEPTH].
template <int DEPTH>
__device__ __forceinline__ u32x4 frame_piece(int q, const uint32_t *sn) {
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w[k] = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int byte = 16 * q + 4 * k + b, pix = byte / DEPTH, ch = byte - pix * DEPTH;
      const int i = pix / 84, j = pix - i * 84;
      w[k] |= tetris_shade<DEPTH>(tetris_cell(sn, tetris_cell_col(j), tetris_cell_row(i)), ch) << (8 * b);
    }
  }
  u32x4 v;
  v.x = w[0];
  v.y = w[1];
  v.z = w[2];
  v.w = w[3];
  return v;
}

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
      a = a < 0 ? 0 : (a > 4 ? 4 : a);
      r = r < 0 ? 0 : (r > R - 1 ? R - 1 : r);
      int rep = tab_rep[r];
      rep = rep < 0 ? 0 : (rep > 255 ? 255 : rep);
      int reward = 0;
      bool over = false;
      tetris_macro_step(cfg, seed, genv, s, board, a, rep + 1, tr, &reward, &over);
      const float rw = (float)reward;
      reward_out[e] = rw;
      over_out[e] = over ? 1.f : 0.f;
      rm_out[(size_t)t * E + e] = rw > 1.f ? 1.f : (rw < -1.f ? -1.f : rw);
      rm_out[((size_t)T + t) * E + e] = over ? 0.f : 1.f;
      if (push_count_out) push_count_out[e] = tr.count;
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
        for (int q = threadIdx.x; q < F16; q += 256) fo[(size_t)j * F16 + q] = frame_piece<DEPTH>(q, sn);
      }
    }
  }
}

int tetris_check(const mt_tetris_config *cfg, int depth, const char *who) {
  MT_CHECK_ARG(cfg != nullptr, "%s: null config", who);
  MT_CHECK_ARG(depth == 1 || depth == 3, "%s: depth must be 1 or 3", who);
  MT_CHECK_ARG(cfg->max_nexts >= 1 && cfg->speed >= 1 && cfg->max_start_wait >= 0 && cfg->max_start_wait <= 30,
               "%s: max_nexts and speed must be >= 1 and max_start_wait in [0, 30]", who);
  return MT_OK;
}

// Host render of one env's stacked state / frames from a trace (the kernel's word and byte functions; every
// word on the exact path, so the kernel's background shortcut is checked against it).
template <int DEPTH>
void host_stack(const TetrisTrace &tr, const uint8_t *prev, uint8_t *out) {
  for (int w = 0; w < 84 * 84 * DEPTH; ++w) {
    uint32_t pw = 0;
    if (tr.count < 4) memcpy(&pw, prev + 4 * (size_t)w, 4);
    const uint32_t v = tetris_word<DEPTH>(w, pw, tr, true);
    memcpy(out + 4 * (size_t)w, &v, 4);
  }
}
template <int DEPTH>
void host_frames(const TetrisTrace &tr, uint8_t *frames) {
  for (int j = 0; j < tr.count; ++j) {
    const uint32_t *sn = tr.snap[(tr.pushes - tr.count + j) & 3];
    uint8_t *f = frames + (size_t)j * 84 * 84 * DEPTH;
    for (int pix = 0; pix < 84 * 84; ++pix)
      for (int ch = 0; ch < DEPTH; ++ch)
        f[pix * DEPTH + ch] =
            (uint8_t)tetris_shade<DEPTH>(tetris_cell(sn, tetris_cell_col(pix % 84), tetris_cell_row(pix / 84)), ch);
  }
}

}  // namespace
}  // namespace mt

using namespace mt;

extern "C" int mt_tetris_reset(const mt_tetris_config *cfg, uint64_t seed, int env0, int E, int depth,
                               mt_tetris_state *state, uint8_t *out_state0, mt_stream_t stream) {
  if (int rc = tetris_check(cfg, depth, "mt_tetris_reset")) return rc;
  MT_CHECK_ARG(E >= 1 && env0 >= 0, "mt_tetris_reset: E must be >= 1 and env0 >= 0");
  MT_CHECK_ARG(state && out_state0, "mt_tetris_reset: null argument");
  MT_CHECK_ARG(((uintptr_t)out_state0 & 15) == 0 && ((uintptr_t)state & 7) == 0, "mt_tetris_reset: misaligned buffer");
  if (depth == 1)
    hipLaunchKernelGGL((tetris_kernel<1, true>), dim3(E), dim3(256), 0, (hipStream_t)stream, *cfg, seed, env0, nullptr, 1,
                       nullptr, nullptr, state, nullptr, out_state0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1);
  else
    hipLaunchKernelGGL((tetris_kernel<3, true>), dim3(E), dim3(256), 0, (hipStream_t)stream, *cfg, seed, env0, nullptr, 1,
                       nullptr, nullptr, state, nullptr, out_state0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1);
  MT_LAUNCHED();
  return MT_OK;
}

extern "C" int mt_tetris_step(const mt_tetris_config *cfg, uint64_t seed, int env0, int E, int depth,
                              const int32_t *tab_rep, int R, const int32_t *a_idx, const int32_t *r_idx,
                              mt_tetris_state *state, const uint8_t *prev, uint8_t *out, uint8_t *frames_out,
                              int32_t *push_count_out, float *reward_out, float *over_out, float *rm_out, int t, int T,
                              mt_stream_t stream) {
  if (int rc = tetris_check(cfg, depth, "mt_tetris_step")) return rc;
  MT_CHECK_ARG(E >= 1 && env0 >= 0 && R >= 1, "mt_tetris_step: E and R must be >= 1 and env0 >= 0");
  MT_CHECK_ARG(T >= 1 && t >= 0 && t < T, "mt_tetris_step: t must be in [0, T)");
  MT_CHECK_ARG(tab_rep && a_idx && r_idx && state && prev && out && reward_out && over_out && rm_out,
               "mt_tetris_step: null argument");
  MT_CHECK_ARG((frames_out == nullptr) == (push_count_out == nullptr),
               "mt_tetris_step: frames_out and push_count_out go together");
  MT_CHECK_ARG(prev != out, "mt_tetris_step: out may not alias prev");
  MT_CHECK_ARG((((uintptr_t)prev | (uintptr_t)out | (uintptr_t)frames_out) & 15) == 0 && ((uintptr_t)state & 7) == 0,
               "mt_tetris_step: misaligned buffer");
  if (depth == 1)
    hipLaunchKernelGGL((tetris_kernel<1, false>), dim3(E), dim3(256), 0, (hipStream_t)stream, *cfg, seed, env0, tab_rep,
                       R, a_idx, r_idx, state, prev, out, frames_out, push_count_out, reward_out, over_out, rm_out, t, T);
  else
    hipLaunchKernelGGL((tetris_kernel<3, false>), dim3(E), dim3(256), 0, (hipStream_t)stream, *cfg, seed, env0, tab_rep,
                       R, a_idx, r_idx, state, prev, out, frames_out, push_count_out, reward_out, over_out, rm_out, t, T);
  MT_LAUNCHED();
  return MT_OK;
}

extern "C" int mt_tetris_reset_host(const mt_tetris_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                                    mt_tetris_state *state, uint8_t *out_state0) {
  if (int rc = tetris_check(cfg, depth, "mt_tetris_reset_host")) return rc;
  MT_CHECK_ARG(state != nullptr, "mt_tetris_reset_host: null state");
  mt_tetris_state st = {};
  TetrisVars s = {};
  TetrisTrace tr = {};
  tetris_reset(*cfg, seed, global_env, s, st.board, tr);
  tetris_store_vars(st, s);
  *state = st;
  if (out_state0) {
    if (depth == 1)
      host_stack<1>(tr, nullptr, out_state0);
    else
      host_stack<3>(tr, nullptr, out_state0);
  }
  return MT_OK;
}

extern "C" int mt_tetris_step_host(const mt_tetris_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                                   const int32_t *tab_rep, int R, int a, int r, mt_tetris_state *state,
                                   const uint8_t *prev, uint8_t *out, uint8_t *frames_out, int32_t *push_count_out,
                                   float *reward_out, float *over_out) {
  if (int rc = tetris_check(cfg, depth, "mt_tetris_step_host")) return rc;
  MT_CHECK_ARG(tab_rep && R >= 1 && state && reward_out && over_out, "mt_tetris_step_host: null argument or R < 1");
  MT_CHECK_ARG(!out || (prev && prev != out), "mt_tetris_step_host: out needs a prev that it does not alias");
  a = a < 0 ? 0 : (a > 4 ? 4 : a);
  r = r < 0 ? 0 : (r > R - 1 ? R - 1 : r);
  int rep = tab_rep[r];
  rep = rep < 0 ? 0 : (rep > 255 ? 255 : rep);
  mt_tetris_state st = *state;
  TetrisVars s = tetris_vars(st);
  for (int y = 0; y < kTetrisRows; ++y) st.board[y] = tetris_board_word(st.board[y]);
  TetrisTrace tr = {};
  int reward;
  bool over;
  tetris_macro_step(*cfg, seed, global_env, s, st.board, a, rep + 1, tr, &reward, &over);
  tetris_store_vars(st, s);
  *state = st;
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
