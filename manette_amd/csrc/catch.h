// Catch (include/manette_hip.h, "Catch": the rule is written out there), integer arithmetic only: the
// env kernel (catch.hip) and mt_catch_*_host share it. A position snapshot packs (paddle_x, ball_x,
// ball_y) into 24 bits; a push = the two snapshots its frame is the maximum of (after sub-frames 3 and
// 4), lo | hi << 32. The trace keeps the last <= 4 pushes as a shift register (q3 newest) indexed by
// constants only, so it lives in scalar registers; a new game restarts it.
#pragma once
#include "common.h"

namespace mt {

constexpr uint64_t kCatchSalt = 0xCA7C4BA11D0FF1E5ULL;
struct CatchTrace {
  uint64_t q0, q1, q2, q3;
  int count;
};
__host__ __device__ __forceinline__ void catch_push(CatchTrace &tr, uint64_t pair) {
  tr.q0 = tr.q1;
  tr.q1 = tr.q2;
  tr.q2 = tr.q3;
  tr.q3 = pair;
  tr.count = tr.count < 4 ? tr.count + 1 : 4;
}
__host__ __device__ __forceinline__ uint32_t catch_snap(const mt_catch_state &s) {
  return (uint32_t)s.paddle_x | ((uint32_t)s.ball_x << 8) | ((uint32_t)s.ball_y << 16);
}
__host__ __device__ __forceinline__ void catch_spawn(uint64_t seed, uint64_t genv, mt_catch_state &s) {
  const uint64_t h = mix64(seed ^ mix64((genv << 40) ^ s.ball_counter) ^ kCatchSalt);
  s.ball_counter += 1;
  s.ball_x = (int32_t)((h & 0xffffffffULL) % 81u);
  s.ball_dx = (int32_t)((h >> 32) % 3u) - 1;
  s.ball_y = 0;
}
// One next(a): returns the push; *reward in {-1, 0, +1}, *over set at an episode end.
__host__ __device__ __forceinline__ uint64_t catch_next(const mt_catch_config &cfg, uint64_t seed, uint64_t genv,
                                                        mt_catch_state &s, int a, int *reward, bool *over) {
  int rw = 0;
  bool ov = false;
  uint32_t s3 = 0;
  for (int f = 0; f < 4; ++f) {
    if (!ov) {
      int px = s.paddle_x + (a == 1 ? -2 : a == 2 ? 2 : 0);
      s.paddle_x = px < 0 ? 0 : (px > 72 ? 72 : px);
      s.ball_y += 2;
      s.ball_x += s.ball_dx;
      if (s.ball_x < 0) {
        s.ball_x = -s.ball_x;
        s.ball_dx = -s.ball_dx;
      } else if (s.ball_x > 80) {
        s.ball_x = 160 - s.ball_x;
        s.ball_dx = -s.ball_dx;
      }
      if (s.ball_y + 3 >= 79) {
        if (s.ball_x < s.paddle_x + 12 && s.ball_x + 4 > s.paddle_x) {
          rw += 1;
        } else {
          rw -= 1;
          s.misses += 1;
        }
        s.balls += 1;
        if (s.misses >= cfg.lives || s.balls >= cfg.max_balls)
          ov = true;
        else
          catch_spawn(seed, genv, s);
      }
    }
    if (f == 2) s3 = catch_snap(s);
  }
  *reward = rw;
  *over = ov;
  return (uint64_t)s3 | ((uint64_t)catch_snap(s) << 32);
}
// A new game (ball_counter kept) and its four next(0): the trace holds the initial state's four frames.
__host__ __device__ __forceinline__ void catch_new_game(const mt_catch_config &cfg, uint64_t seed, uint64_t genv,
                                                        mt_catch_state &s, CatchTrace &tr) {
  s.paddle_x = 36;
  s.misses = 0;
  s.balls = 0;
  catch_spawn(seed, genv, s);
  tr.count = 0;
  for (int i = 0; i < 4; ++i) {
    int rw;
    bool ov;
    catch_push(tr, catch_next(cfg, seed, genv, s, 0, &rw, &ov));
  }
}
// One macro-step: n = tab_rep[r] + 1 times next(a), stopping at the first episode end (then a new game).
__host__ __device__ __forceinline__ void catch_macro_step(const mt_catch_config &cfg, uint64_t seed, uint64_t genv,
                                                          mt_catch_state &s, int a, int n, CatchTrace &tr,
                                                          int *reward, bool *over) {
  int sum = 0;
  bool ended = false;
  tr.count = 0;
  for (int i = 0; i < n && !ended; ++i) {
    int rw;
    catch_push(tr, catch_next(cfg, seed, genv, s, a, &rw, &ended));
    sum += rw;
  }
  if (ended) catch_new_game(cfg, seed, genv, s, tr);
  *reward = sum;
  *over = ended;
}
// Render: the value of channel ch of pixel (x, y) under one snapshot, and a push's frame value.
template <int DEPTH>
__host__ __device__ __forceinline__ uint32_t catch_render(int x, int y, int ch, uint32_t snap) {
  const int px = (int)(snap & 0xffu), bx = (int)((snap >> 8) & 0xffu), by = (int)((snap >> 16) & 0xffu);
  const uint32_t ball = DEPTH == 1 ? 255u : (ch == 0 ? 255u : 64u);
  const uint32_t pad = DEPTH == 1 ? 160u : (ch == 1 ? 255u : 64u);
  const bool in_ball = (unsigned)(x - bx) < 4u && (unsigned)(y - by) < 4u;
  const bool in_pad = (unsigned)(x - px) < 12u && (unsigned)(y - 79) < 3u;
  return in_ball ? ball : (in_pad ? pad : 0u);
}
template <int DEPTH>
__host__ __device__ __forceinline__ uint32_t catch_value(int x, int y, int ch, uint64_t pair) {
  const uint32_t a = catch_render<DEPTH>(x, y, ch, (uint32_t)pair), b = catch_render<DEPTH>(x, y, ch, (uint32_t)(pair >> 32));
  return a > b ? a : b;
}
// 32-bit word w of an env's stacked state = the four stack bytes (oldest in the low byte) of channel
// w % DEPTH of pixel w / DEPTH: prev's word shifted down by the pushes, the new values above it.
template <int DEPTH>
__host__ __device__ __forceinline__ uint32_t catch_word(int w, uint32_t prev_word, const CatchTrace &tr) {
  const int pix = w / DEPTH, ch = w - pix * DEPTH;
  const int y = pix / 84, x = pix - y * 84;
  uint32_t v = tr.count < 4 ? prev_word >> (8 * tr.count) : 0u;
  if (tr.count >= 4) v |= catch_value<DEPTH>(x, y, ch, tr.q0);
  if (tr.count >= 3) v |= catch_value<DEPTH>(x, y, ch, tr.q1) << 8;
  if (tr.count >= 2) v |= catch_value<DEPTH>(x, y, ch, tr.q2) << 16;
  if (tr.count >= 1) v |= catch_value<DEPTH>(x, y, ch, tr.q3) << 24;
  return v;
}
// Push j (oldest first, j < tr.count) of the trace.
__host__ __device__ __forceinline__ uint64_t catch_trace_push(const CatchTrace &tr, int j) {
  const int k = 4 - tr.count + j;
  return k == 0 ? tr.q0 : (k == 1 ? tr.q1 : (k == 2 ? tr.q2 : tr.q3));
}

}  // namespace mt
