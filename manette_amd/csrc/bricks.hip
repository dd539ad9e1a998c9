// Bricks, the second device-resident environment (include/manette_hip.h, "Bricks"; the rule: bricks.h).
// catch_kernel's shape: one kernel per macro-step runs the game logic of every env, renders its pushed
// frames and writes the next stacked state straight into the rollout's state ring.
#include "bricks.h"

namespace mt {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t sgpr_u(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t sgpr_u64(uint64_t v) {
  return (uint64_t)sgpr_u((uint32_t)v) | ((uint64_t)sgpr_u((uint32_t)(v >> 32)) << 32);
}

// The rows of the field (an 84-bit mask in two words) that any sprite of a pushed snapshot touches.
struct Rows84 {
  uint64_t lo, hi;
};
// bits (<= 4 wide) are set from `start` <= 81
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

// The bytes of 16-byte piece q of push p's own frame [84][84][DEPTH].
template <int DEPTH>
__device__ __forceinline__ u32x4 frame_piece(int q, const BricksPush &p) {
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w[k] = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int byte = 16 * q + 4 * k + b, pix = byte / DEPTH, ch = byte - pix * DEPTH;
      const int y = pix / 84, x = pix - y * 84;
      w[k] |= bricks_value<DEPTH>(x, y, ch, bricks_pixel<DEPTH>(x, y, ch), p) << (8 * b);
    }
  }
  u32x4 v;
  v.x = w[0];
  v.y = w[1];
  v.z = w[2];
  v.w = w[3];
  return v;
}
template <int DEPTH>
__device__ __forceinline__ void write_frame(u32x4 *dst, const BricksPush &p) {
  for (int q = threadIdx.x; q < 84 * 84 * DEPTH / 16; q += 256) dst[q] = frame_piece<DEPTH>(q, p);
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
    a = a < 0 ? 0 : (a > 3 ? 3 : a);
    r = r < 0 ? 0 : (r > R - 1 ? R - 1 : r);
    int rep = sgpr(tab_rep[r]);
    rep = rep < 0 ? 0 : (rep > 255 ? 255 : rep);
    bricks_macro_step(cfg, seed, genv, s, a, rep + 1, tr, &reward, &over);
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

int bricks_check(const mt_bricks_config *cfg, int depth, const char *who) {
  MT_CHECK_ARG(cfg != nullptr, "%s: null config", who);
  MT_CHECK_ARG(depth == 1 || depth == 3, "%s: depth must be 1 or 3", who);
  MT_CHECK_ARG(cfg->lives >= 1 && cfg->max_nexts >= 1 && cfg->serve_wait >= 0,
               "%s: lives and max_nexts must be >= 1 and serve_wait >= 0", who);
  return MT_OK;
}

// Host render of one env's stacked state / frames from a trace (the kernel's word and byte functions).
template <int DEPTH>
void host_stack(const BricksTrace &tr, const uint8_t *prev, uint8_t *out) {
  for (int w = 0; w < 84 * 84 * DEPTH; ++w) {
    uint32_t pw = 0;
    if (tr.count < 4) memcpy(&pw, prev + 4 * (size_t)w, 4);
    const uint32_t v = bricks_word<DEPTH>(w, pw, tr);
    memcpy(out + 4 * (size_t)w, &v, 4);
  }
}
template <int DEPTH>
void host_frames(const BricksTrace &tr, uint8_t *frames) {
  const BricksPush *q[4] = {&tr.q0, &tr.q1, &tr.q2, &tr.q3};
  for (int j = 0; j < tr.count; ++j) {
    const BricksPush &p = *q[4 - tr.count + j];
    uint8_t *f = frames + (size_t)j * 84 * 84 * DEPTH;
    for (int pix = 0; pix < 84 * 84; ++pix)
      for (int ch = 0; ch < DEPTH; ++ch) {
        const int x = pix % 84, y = pix / 84;
        f[pix * DEPTH + ch] = (uint8_t)bricks_value<DEPTH>(x, y, ch, bricks_pixel<DEPTH>(x, y, ch), p);
      }
  }
}

}  // namespace
}  // namespace mt

using namespace mt;

extern "C" int mt_bricks_reset(const mt_bricks_config *cfg, uint64_t seed, int env0, int E, int depth,
                               mt_bricks_state *state, uint8_t *out_state0, mt_stream_t stream) {
  if (int rc = bricks_check(cfg, depth, "mt_bricks_reset")) return rc;
  MT_CHECK_ARG(E >= 1 && env0 >= 0, "mt_bricks_reset: E must be >= 1 and env0 >= 0");
  MT_CHECK_ARG(state && out_state0, "mt_bricks_reset: null argument");
  MT_CHECK_ARG(((uintptr_t)out_state0 & 15) == 0 && ((uintptr_t)state & 7) == 0, "mt_bricks_reset: misaligned buffer");
  if (depth == 1)
    hipLaunchKernelGGL((bricks_kernel<1, true>), dim3(E), dim3(256), 0, (hipStream_t)stream, *cfg, seed, env0, nullptr, 1,
                       nullptr, nullptr, state, nullptr, out_state0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1);
  else
    hipLaunchKernelGGL((bricks_kernel<3, true>), dim3(E), dim3(256), 0, (hipStream_t)stream, *cfg, seed, env0, nullptr, 1,
                       nullptr, nullptr, state, nullptr, out_state0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1);
  MT_LAUNCHED();
  return MT_OK;
}

extern "C" int mt_bricks_step(const mt_bricks_config *cfg, uint64_t seed, int env0, int E, int depth,
                              const int32_t *tab_rep, int R, const int32_t *a_idx, const int32_t *r_idx,
                              mt_bricks_state *state, const uint8_t *prev, uint8_t *out, uint8_t *frames_out,
                              int32_t *push_count_out, float *reward_out, float *over_out, float *rm_out, int t, int T,
                              mt_stream_t stream) {
  if (int rc = bricks_check(cfg, depth, "mt_bricks_step")) return rc;
  MT_CHECK_ARG(E >= 1 && env0 >= 0 && R >= 1, "mt_bricks_step: E and R must be >= 1 and env0 >= 0");
  MT_CHECK_ARG(T >= 1 && t >= 0 && t < T, "mt_bricks_step: t must be in [0, T)");
  MT_CHECK_ARG(tab_rep && a_idx && r_idx && state && prev && out && reward_out && over_out && rm_out,
               "mt_bricks_step: null argument");
  MT_CHECK_ARG((frames_out == nullptr) == (push_count_out == nullptr),
               "mt_bricks_step: frames_out and push_count_out go together");
  MT_CHECK_ARG(prev != out, "mt_bricks_step: out may not alias prev");
  MT_CHECK_ARG((((uintptr_t)prev | (uintptr_t)out | (uintptr_t)frames_out) & 15) == 0 && ((uintptr_t)state & 7) == 0,
               "mt_bricks_step: misaligned buffer");
  if (depth == 1)
    hipLaunchKernelGGL((bricks_kernel<1, false>), dim3(E), dim3(256), 0, (hipStream_t)stream, *cfg, seed, env0, tab_rep,
                       R, a_idx, r_idx, state, prev, out, frames_out, push_count_out, reward_out, over_out, rm_out, t, T);
  else
    hipLaunchKernelGGL((bricks_kernel<3, false>), dim3(E), dim3(256), 0, (hipStream_t)stream, *cfg, seed, env0, tab_rep,
                       R, a_idx, r_idx, state, prev, out, frames_out, push_count_out, reward_out, over_out, rm_out, t, T);
  MT_LAUNCHED();
  return MT_OK;
}

extern "C" int mt_bricks_reset_host(const mt_bricks_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                                    mt_bricks_state *state, uint8_t *out_state0) {
  (void)seed;
  (void)global_env;  // (a new game draws nothing: the first serve hashes them)
  if (int rc = bricks_check(cfg, depth, "mt_bricks_reset_host")) return rc;
  MT_CHECK_ARG(state != nullptr, "mt_bricks_reset_host: null state");
  mt_bricks_state s = {};
  BricksTrace tr = {};
  bricks_new_game(*cfg, s, tr);
  *state = s;
  if (out_state0) {
    if (depth == 1)
      host_stack<1>(tr, nullptr, out_state0);
    else
      host_stack<3>(tr, nullptr, out_state0);
  }
  return MT_OK;
}

extern "C" int mt_bricks_step_host(const mt_bricks_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                                   const int32_t *tab_rep, int R, int a, int r, mt_bricks_state *state,
                                   const uint8_t *prev, uint8_t *out, uint8_t *frames_out, int32_t *push_count_out,
                                   float *reward_out, float *over_out) {
  if (int rc = bricks_check(cfg, depth, "mt_bricks_step_host")) return rc;
  MT_CHECK_ARG(tab_rep && R >= 1 && state && reward_out && over_out, "mt_bricks_step_host: null argument or R < 1");
  MT_CHECK_ARG(!out || (prev && prev != out), "mt_bricks_step_host: out needs a prev that it does not alias");
  a = a < 0 ? 0 : (a > 3 ? 3 : a);
  r = r < 0 ? 0 : (r > R - 1 ? R - 1 : r);
  int rep = tab_rep[r];
  rep = rep < 0 ? 0 : (rep > 255 ? 255 : rep);
  mt_bricks_state s = *state;
  s.bricks_hi &= kBricksFullHi;
  s.reserved = 0;
  BricksTrace tr = {};
  int reward;
  bool over;
  bricks_macro_step(*cfg, seed, global_env, s, a, rep + 1, tr, &reward, &over);
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
