// Bricks (include/manette_hip.h, "Bricks": the rule is written out there), integer arithmetic only: the
// env kernel (bricks.hip) and mt_bricks_*_host share these functions. A snapshot is what one render
// needs: the positions (paddle_x, ball_x, ball_y packed into 24 bits) and the 84-bit brick bitmap. A push
// keeps BOTH snapshots its frame is the maximum of (after sub-frames 3 and 4), bitmaps included: the
// maximum of two renders is not a function of the bitmaps' union (where the ball of one snapshot lies
// over a brick that only that snapshot still has, the exact value is the ball's colour, the union's is
// the per-channel maximum of ball and brick). The trace keeps the last <= 4 pushes as a shift register
// (q3 newest) indexed by constants only, so its 32 words live in scalar registers.
#pragma once
#include "common.h"

namespace mt {

constexpr uint64_t kBricksSalt = 0xB41C5B0117A11E75ULL;
constexpr uint64_t kBricksFullLo = ~0ULL;
constexpr uint32_t kBricksFullHi = 0xFFFFFu;  // bits 64..83

struct BricksSnap {
  uint64_t lo;
  uint32_t hi, pos;
};
struct BricksPush {
  BricksSnap a, b;  // after sub-frame 3, after sub-frame 4
};
struct BricksTrace {
  BricksPush q0, q1, q2, q3;
  int count;
};
__host__ __device__ __forceinline__ void bricks_push(BricksTrace &tr, const BricksPush &p) {
  tr.q0 = tr.q1;
  tr.q1 = tr.q2;
  tr.q2 = tr.q3;
  tr.q3 = p;
  tr.count = tr.count < 4 ? tr.count + 1 : 4;
}
__host__ __device__ __forceinline__ BricksSnap bricks_snap(const mt_bricks_state &s) {
  BricksSnap p;
  p.lo = s.bricks_lo;
  p.hi = s.bricks_hi;
  p.pos = (uint32_t)s.paddle_x | ((uint32_t)s.ball_x << 8) | ((uint32_t)s.ball_y << 16);
  return p;
}
// Bit k (0..83) of a bitmap; no shift reaches the width of its operand.
__host__ __device__ __forceinline__ bool bricks_bit(uint64_t lo, uint32_t hi, int k) {
  return k < 64 ? ((lo >> (k & 63)) & 1ull) != 0 : ((hi >> ((k - 64) & 31)) & 1u) != 0;
}
// The 14 bits of brick row r (bit 63 / 64 falls inside row 4).
__host__ __device__ __forceinline__ uint32_t bricks_row_bits(uint64_t lo, uint32_t hi, int r) {
  const int start = 14 * r;
  uint64_t v;
  if (start + 14 <= 64)
    v = lo >> start;
  else if (start >= 64)
    v = (uint64_t)(hi >> (start - 64));
  else
    v = (lo >> start) | ((uint64_t)hi << (64 - start));
  return (uint32_t)v & 0x3fffu;
}
__host__ __device__ __forceinline__ int bricks_dx(int i) { return i < 2 ? i - 2 : i - 1; }  // (-2, -1, +1, +2)[i]

__host__ __device__ __forceinline__ void bricks_park(mt_bricks_state &s) {
  s.ball_dy = 0;
  s.ball_dx = 0;
  s.ball_x = s.paddle_x + 7;
  s.ball_y = 77;
}
// One next(a): returns the push; *reward in 0..4, *over set at an episode end.
__host__ __device__ __forceinline__ BricksPush bricks_next(const mt_bricks_config &cfg, uint64_t seed, uint64_t genv,
                                                           mt_bricks_state &s, int a, int *reward, bool *over) {
  int rw = 0;
  bool ov = false;
  if (s.ball_dy == 0) {
    if (a == 1 || s.wait >= cfg.serve_wait) {
      const uint64_t h = mix64(seed ^ mix64((genv << 40) ^ s.serve_counter) ^ kBricksSalt);
      s.serve_counter += 1;
      s.ball_x = s.paddle_x + 7;
      s.ball_y = 36;
      s.ball_dy = 2;
      s.ball_dx = bricks_dx((int)((h >> 32) & 3u));
    } else {
      s.wait += 1;
    }
  }
  BricksPush p;
  for (int f = 0; f < 4; ++f) {
    if (!ov) {
      const int px = s.paddle_x + (a == 2 ? 3 : a == 3 ? -3 : 0);
      s.paddle_x = px < 0 ? 0 : (px > 68 ? 68 : px);
      if (s.ball_dy == 0) {
        s.ball_x = s.paddle_x + 7;
      } else {
        s.ball_x += s.ball_dx;
        if (s.ball_x < 0) {
          s.ball_x = -s.ball_x;
          s.ball_dx = -s.ball_dx;
        } else if (s.ball_x > 82) {
          s.ball_x = 164 - s.ball_x;
          s.ball_dx = -s.ball_dx;
        }
        s.ball_y += s.ball_dy;
        if (s.ball_y < 0) {
          s.ball_y = -s.ball_y;
          s.ball_dy = -s.ball_dy;
        }
        const int cy = s.ball_y + (s.ball_dy > 0 ? 1 : 0), cx = s.ball_x + (s.ball_dx > 0 ? 1 : 0);
        if (cy >= 16 && cy < 34) {
          const int k = 14 * ((cy - 16) / 3) + cx / 6;
          if (bricks_bit(s.bricks_lo, s.bricks_hi, k)) {
            if (k < 64)
              s.bricks_lo &= ~(1ull << (k & 63));
            else
              s.bricks_hi &= ~(1u << ((k - 64) & 31));
            rw += 1;
            s.ball_dy = -s.ball_dy;
            if (s.bricks_lo == 0 && s.bricks_hi == 0) {
              s.bricks_lo = kBricksFullLo;
              s.bricks_hi = kBricksFullHi;
            }
          }
        }
        if (s.ball_dy > 0 && s.ball_y + 1 >= 79) {
          const int off = s.ball_x + 1 - s.paddle_x;
          if (off >= 0 && off <= 16) {
            const int i = 4 * off / 17;
            s.ball_dy = -2;
            s.ball_y = 77;
            s.ball_dx = bricks_dx(i > 3 ? 3 : i);
          } else {
            s.lives -= 1;
            if (s.lives <= 0) {
              ov = true;
            } else {
              bricks_park(s);
              s.wait = 0;
            }
          }
        }
      }
    }
    if (f == 2) p.a = bricks_snap(s);
  }
  p.b = bricks_snap(s);
  s.nexts += 1;
  if (s.nexts >= cfg.max_nexts) ov = true;
  *reward = rw;
  *over = ov;
  return p;
}
// A new game (serve_counter kept): nothing is played, the trace holds four copies of its position.
__host__ __device__ __forceinline__ void bricks_new_game(const mt_bricks_config &cfg, mt_bricks_state &s,
                                                         BricksTrace &tr) {
  s.paddle_x = 34;
  s.lives = cfg.lives;
  s.nexts = 0;
  s.wait = 0;
  s.bricks_lo = kBricksFullLo;
  s.bricks_hi = kBricksFullHi;
  s.reserved = 0;
  bricks_park(s);
  BricksPush p;
  p.a = p.b = bricks_snap(s);
  tr.q0 = tr.q1 = tr.q2 = tr.q3 = p;
  tr.count = 4;
}
// One macro-step: n = tab_rep[r] + 1 times next(a), stopping at the first episode end (then a new game).
__host__ __device__ __forceinline__ void bricks_macro_step(const mt_bricks_config &cfg, uint64_t seed, uint64_t genv,
                                                           mt_bricks_state &s, int a, int n, BricksTrace &tr,
                                                           int *reward, bool *over) {
  int sum = 0;
  bool ended = false;
  tr.count = 0;
  for (int i = 0; i < n && !ended; ++i) {
    int rw;
    bricks_push(tr, bricks_next(cfg, seed, genv, s, a, &rw, &ended));
    sum += rw;
  }
  if (ended) bricks_new_game(cfg, s, tr);
  *reward = sum;
  *over = ended;
}

// What a pixel needs of the wall, the same for every snapshot: its brick bit (-1 outside rows 16..33)
// and that brick row's colour in channel ch (six bytes packed per channel, row 0 lowest).
struct BricksPixel {
  int k;
  uint32_t brick;
};
template <int DEPTH>
__host__ __device__ __forceinline__ BricksPixel bricks_pixel(int x, int y, int ch) {
  BricksPixel q = {-1, 0u};
  if ((unsigned)(y - 16) < 18u) {
    const int r = (y - 16) / 3;
    q.k = 14 * r + x / 6;
    if (DEPTH == 1) {
      q.brick = 90u + 20u * (uint32_t)r;
    } else {
      const uint64_t pk = ch == 0 ? 0x4248A2B4C6C8ULL : (ch == 1 ? 0x48A0A27A6C48ULL : 0xC8482A303A48ULL);
      q.brick = (uint32_t)(pk >> (8 * r)) & 0xffu;
    }
  }
  return q;
}
// One render: the ball over the bricks over the paddle.
template <int DEPTH>
__host__ __device__ __forceinline__ uint32_t bricks_render(int x, int y, int ch, const BricksPixel &q,
                                                           const BricksSnap &sn) {
  const int px = (int)(sn.pos & 0xffu), bx = (int)((sn.pos >> 8) & 0xffu), by = (int)((sn.pos >> 16) & 0xffu);
  const uint32_t ball = DEPTH == 1 ? 255u : (ch == 0 ? 255u : 64u);
  const uint32_t pad = DEPTH == 1 ? 160u : (ch == 1 ? 255u : 64u);
  const bool in_ball = (unsigned)(x - bx) < 2u && (unsigned)(y - by) < 2u;
  const bool in_brick = q.k >= 0 && bricks_bit(sn.lo, sn.hi, q.k);
  const bool in_pad = (unsigned)(x - px) < 16u && (unsigned)(y - 79) < 3u;
  return in_ball ? ball : (in_brick ? q.brick : (in_pad ? pad : 0u));
}
template <int DEPTH>
__host__ __device__ __forceinline__ uint32_t bricks_value(int x, int y, int ch, const BricksPixel &q,
                                                          const BricksPush &p) {
  const uint32_t a = bricks_render<DEPTH>(x, y, ch, q, p.a), b = bricks_render<DEPTH>(x, y, ch, q, p.b);
  return a > b ? a : b;
}
// 32-bit word w of an env's stacked state = the four stack bytes (oldest in the low byte) of channel
// w % DEPTH of pixel w / DEPTH: prev's word shifted down by the pushes, the new values above it.
template <int DEPTH>
__host__ __device__ __forceinline__ uint32_t bricks_word(int w, uint32_t prev_word, const BricksTrace &tr) {
  const int pix = w / DEPTH, ch = w - pix * DEPTH;
  const int y = pix / 84, x = pix - y * 84;
  const BricksPixel q = bricks_pixel<DEPTH>(x, y, ch);
  uint32_t v = tr.count < 4 ? prev_word >> (8 * tr.count) : 0u;
  if (tr.count >= 4) v |= bricks_value<DEPTH>(x, y, ch, q, tr.q0);
  if (tr.count >= 3) v |= bricks_value<DEPTH>(x, y, ch, q, tr.q1) << 8;
  if (tr.count >= 2) v |= bricks_value<DEPTH>(x, y, ch, q, tr.q2) << 16;
  if (tr.count >= 1) v |= bricks_value<DEPTH>(x, y, ch, q, tr.q3) << 24;
  return v;
}

}  // namespace mt
