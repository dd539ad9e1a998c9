// Tetris (include/manette_hip.h, "Tetris": the rule is written out there), integer arithmetic only: the
// env kernel (tetris.hip) and mt_tetris_*_host share these functions. The board is 22 words (a row per
// word, 3 bits per cell), indexed by run-time rows, so it is never held in a private array: the rule works
// on the state's scalar fields (TetrisVars: registers in the kernel) and through pointers to the board and
// to the trace, which the kernel keeps in LDS and the host on its stack.
// A snapshot is what one render needs: the 22 board words and one word packing the falling piece (id,
// rotation, x, y) and the next piece, with their two bit matrices in another. The trace keeps the last <= 4 pushed snapshots as a ring.
#pragma once
#include "common.h"

namespace mt {

constexpr uint64_t kTetrisSalt = 0x7E7215B10C5D20F7ULL;
constexpr uint64_t kTetrisWaitSalt = 0x57A27F0A17C0FFEEULL;
constexpr uint32_t kTetrisRowMask = 0x3fffffffu;  // 10 cells x 3 bits
constexpr uint32_t kTetrisCellLsb = 0x09249249u;  // bit 0 of each of the 10 cells
constexpr int kTetrisRows = 22, kTetrisCols = 10, kTetrisSnapWords = 24;

// The scalar fields of mt_tetris_state.
struct TetrisVars {
  int piece, rot, x, y, next_piece, level, lines, speed, speed_counter, nexts;
  uint64_t piece_counter;
};
struct TetrisTrace {
  uint32_t snap[4][kTetrisSnapWords];  // push k of the macro-step at slot k & 3: board[22], pieces, their matrices
  int pushes, count;                   // count = min(pushes, 4)
  uint32_t live;                       // bit cy: cell row cy shows more than background in some pushed snapshot
};

// The 4 x 4 bit matrix (bit 4 r + c = row r, column c) of shape id under rot rotations: 16 bits per rotation.
__host__ __device__ __forceinline__ uint32_t tetris_mask(int id, int rot) {
  const uint64_t pk = id == 1   ? 0x0232007201310027ULL
                      : id == 2 ? 0x0231003602310036ULL
                      : id == 3 ? 0x0132006301320063ULL
                      : id == 4 ? 0x0113004703220071ULL
                      : id == 5 ? 0x0311001702230074ULL
                      : id == 6 ? 0x1111000F1111000FULL
                                : 0x0033003300330033ULL;
  return (uint32_t)(pk >> (16 * (rot & 3))) & 0xffffu;
}
__host__ __device__ __forceinline__ int tetris_width(uint32_t m) {
  const uint32_t c = (m | (m >> 4) | (m >> 8) | (m >> 12)) & 0xfu;
  return (c & 8u) ? 4 : ((c & 4u) ? 3 : ((c & 2u) ? 2 : 1));
}
// The 4 cells of a matrix row spread to 3 bits each, times v (1..7).
__host__ __device__ __forceinline__ uint32_t tetris_spread(uint32_t rb, uint32_t v) {
  return ((rb & 1u) | ((rb & 2u) << 2) | ((rb & 4u) << 4) | ((rb & 8u) << 6)) * v;
}
// x in [0, 9], y >= 0: no shift reaches 32, no row outside the board is read.
__host__ __device__ __forceinline__ bool tetris_collides(const uint32_t *board, uint32_t m, int x, int y) {
  bool hit = false;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t rb = (m >> (4 * r)) & 0xfu;
    if (rb != 0) {
      const int by = y + r;
      const uint64_t e = (uint64_t)tetris_spread(rb, 7u) << (3 * x);
      hit = hit || by >= kTetrisRows || (e >> 30) != 0 || (board[by < kTetrisRows ? by : kTetrisRows - 1] & (uint32_t)e) != 0;
    }
  }
  return hit;
}
__host__ __device__ __forceinline__ uint64_t tetris_hash(uint64_t seed, uint64_t genv, uint64_t counter, uint64_t salt) {
  return mix64(seed ^ mix64((genv << 40) ^ counter) ^ salt);
}
__host__ __device__ __forceinline__ int tetris_draw(uint64_t seed, uint64_t genv, TetrisVars &s) {
  const uint64_t h = tetris_hash(seed, genv, s.piece_counter, kTetrisSalt);
  s.piece_counter += 1;
  return 1 + (int)(h % 7u);
}
// The next piece becomes the falling one; returns whether it collides (game over).
__host__ __device__ __forceinline__ bool tetris_spawn(uint64_t seed, uint64_t genv, TetrisVars &s, const uint32_t *board) {
  s.piece = s.next_piece;
  s.rot = 0;
  const uint32_t m = tetris_mask(s.piece, 0);
  s.x = tetris_width(m) == 2 ? 4 : 3;
  s.y = 0;
  s.next_piece = tetris_draw(seed, genv, s);
  return tetris_collides(board, m, s.x, s.y);
}
// Full rows removed, the rows above moving down; returns their number.
__host__ __device__ __forceinline__ int tetris_remove_rows(uint32_t *board) {
  int d = kTetrisRows - 1, n = 0;
  for (int i = kTetrisRows - 1; i >= 0; --i) {
    const uint32_t b = board[i], t = b | (b >> 1) | (b >> 2);
    if ((t & kTetrisCellLsb) == kTetrisCellLsb) {
      n += 1;
    } else {
      board[d] = b;  // (d >= i: nothing unread is overwritten)
      d -= 1;
    }
  }
  for (; d >= 0; --d) board[d] = 0u;
  return n;
}
__host__ __device__ __forceinline__ void tetris_drop(uint64_t seed, uint64_t genv, TetrisVars &s, uint32_t *board,
                                                     bool manual, int *reward, bool *gameover) {
  if (*gameover) return;
  if (manual) *reward += 1;
  s.y += 1;
  const uint32_t m = tetris_mask(s.piece, s.rot);
  if (!tetris_collides(board, m, s.x, s.y)) return;
  const uint32_t id = (uint32_t)s.piece;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t rb = (m >> (4 * r)) & 0xfu;
    const int by = s.y - 1 + r;
    if (rb != 0 && by < kTetrisRows) board[by] |= (tetris_spread(rb, id) << (3 * s.x)) & kTetrisRowMask;
  }
  *gameover = tetris_spawn(seed, genv, s, board);
  const int n = tetris_remove_rows(board);
  s.lines += n;
  *reward += (n <= 0 ? 0 : (n == 1 ? 40 : (n == 2 ? 100 : (n == 3 ? 300 : 1200)))) * s.level;
  if (s.lines >= 6 * s.level) {
    s.level += 1;
    s.speed = s.speed > 1 ? s.speed - 1 : 1;
  }
}
// One act(a): the action, gravity, speed_counter. *reward is added to, *gameover set.
__host__ __device__ __forceinline__ void tetris_act(uint64_t seed, uint64_t genv, TetrisVars &s, uint32_t *board, int a,
                                                    int *reward, bool *gameover) {
  if (a == 1 || a == 2) {
    const uint32_t m = tetris_mask(s.piece, s.rot);
    const int hi = kTetrisCols - tetris_width(m);
    int nx = s.x + (a == 1 ? -1 : 1);
    nx = nx < 0 ? 0 : (nx > hi ? hi : nx);
    if (!tetris_collides(board, m, nx, s.y)) s.x = nx;
  } else if (a == 3) {
    tetris_drop(seed, genv, s, board, true, reward, gameover);
  } else if (a == 4) {
    if (!tetris_collides(board, tetris_mask(s.piece, s.rot + 1), s.x, s.y)) s.rot = (s.rot + 1) & 3;
  }
  if (s.speed_counter % s.speed == 0) tetris_drop(seed, genv, s, board, false, reward, gameover);
  s.speed_counter += 1;
}
// The trace's counters while a macro-step is played (registers in the kernel); tetris_trace_close stores them.
struct TetrisRun {
  int pushes;
  uint32_t live;
};
__host__ __device__ __forceinline__ void tetris_push(TetrisTrace &tr, TetrisRun &run, const TetrisVars &s,
                                                     const uint32_t *board) {
  uint32_t *sn = tr.snap[run.pushes & 3];
  uint32_t live = 0xCu | ((0xFu << s.y) & 0x3fffffu);  // the next piece's rows 2..3, the falling piece's (<= 4)
  for (int y = 0; y < kTetrisRows; ++y) {
    const uint32_t b = board[y];
    sn[y] = b;
    live |= (b != 0u ? 1u : 0u) << y;
  }
  sn[22] = (uint32_t)s.piece | ((uint32_t)s.x << 4) | ((uint32_t)s.y << 8) | ((uint32_t)s.next_piece << 16);
  sn[23] = tetris_mask(s.piece, s.rot) | (tetris_mask(s.next_piece, 0) << 16);
  run.live |= live;
  run.pushes += 1;
}
__host__ __device__ __forceinline__ void tetris_trace_close(TetrisTrace &tr, const TetrisRun &run) {
  tr.pushes = run.pushes;
  tr.count = run.pushes < 4 ? run.pushes : 4;
  tr.live = run.live;
}
// The scalar fields of a state; one from outside the rule cannot index or shift out of range (the board
// words are masked where they are copied: tetris_board_word).
__host__ __device__ __forceinline__ TetrisVars tetris_vars(const mt_tetris_state &st) {
  TetrisVars s;
  s.piece = st.piece < 1 ? 1 : (st.piece > 7 ? 7 : st.piece);
  s.next_piece = st.next_piece < 1 ? 1 : (st.next_piece > 7 ? 7 : st.next_piece);
  s.rot = st.rot < 0 ? 0 : (st.rot > 3 ? 3 : st.rot);
  s.x = st.x < 0 ? 0 : (st.x > 9 ? 9 : st.x);
  s.y = st.y < 0 ? 0 : (st.y > 21 ? 21 : st.y);
  s.level = st.level < 1 ? 1 : (st.level > (1 << 20) ? (1 << 20) : st.level);  // (1200 x level fits)
  s.lines = st.lines < 0 ? 0 : (st.lines > (1 << 28) ? (1 << 28) : st.lines);
  s.speed = st.speed < 1 ? 1 : st.speed;
  s.speed_counter = st.speed_counter < 0 ? 0 : (st.speed_counter > (1 << 30) ? (1 << 30) : st.speed_counter);
  s.nexts = st.nexts < 0 ? 0 : (st.nexts > (1 << 30) ? (1 << 30) : st.nexts);
  s.piece_counter = st.piece_counter;
  return s;
}
__host__ __device__ __forceinline__ uint32_t tetris_board_word(uint32_t w) { return w & kTetrisRowMask; }
__host__ __device__ __forceinline__ void tetris_store_vars(mt_tetris_state &st, const TetrisVars &s) {
  st.piece = s.piece;
  st.rot = s.rot;
  st.x = s.x;
  st.y = s.y;
  st.next_piece = s.next_piece;
  st.level = s.level;
  st.lines = s.lines;
  st.speed = s.speed;
  st.speed_counter = s.speed_counter;
  st.nexts = s.nexts;
  st.piece_counter = s.piece_counter;
}
// A new game (piece_counter and next_piece kept): w + 4 act(0), the last four pushed.
__host__ __device__ __forceinline__ void tetris_new_game(const mt_tetris_config &cfg, uint64_t seed, uint64_t genv,
                                                         TetrisVars &s, uint32_t *board, TetrisTrace &tr) {
  for (int y = 0; y < kTetrisRows; ++y) board[y] = 0u;
  (void)tetris_spawn(seed, genv, s, board);
  s.level = 1;
  s.lines = 0;
  s.speed = cfg.speed;
  s.speed_counter = 0;
  const int w = (int)(tetris_hash(seed, genv, s.piece_counter, kTetrisWaitSalt) % (uint64_t)(cfg.max_start_wait + 1));
  TetrisRun run = {0, 0u};
  for (int k = 0; k < w + 4; ++k) {
    int rw = 0;
    bool ov = false;
    tetris_act(seed, genv, s, board, 0, &rw, &ov);
    if (k >= w) tetris_push(tr, run, s, board);
  }
  tetris_trace_close(tr, run);
  s.nexts = 0;
}
// A reset: the first next piece is draw 0, then a new game.
__host__ __device__ __forceinline__ void tetris_reset(const mt_tetris_config &cfg, uint64_t seed, uint64_t genv,
                                                      TetrisVars &s, uint32_t *board, TetrisTrace &tr) {
  s.piece_counter = 0;
  s.next_piece = tetris_draw(seed, genv, s);
  tetris_new_game(cfg, seed, genv, s, board, tr);
}
// One macro-step: n times next(a), stopping at the first episode end (then a new game).
__host__ __device__ __forceinline__ void tetris_macro_step(const mt_tetris_config &cfg, uint64_t seed, uint64_t genv,
                                                           TetrisVars &s, uint32_t *board, int a, int n, TetrisTrace &tr,
                                                           int *reward, bool *over) {
  int sum = 0;
  bool ended = false;
  TetrisRun run = {0, 0u};
  for (int i = 0; i < n && !ended; ++i) {
    tetris_act(seed, genv, s, board, a, &sum, &ended);
    s.nexts += 1;
    if (s.nexts >= cfg.max_nexts) ended = true;
    if (n - 1 - i < 4) tetris_push(tr, run, s, board);
  }
  if (ended)
    tetris_new_game(cfg, seed, genv, s, board, tr);
  else
    tetris_trace_close(tr, run);
  *reward = sum;
  *over = ended;
}

// ---- render ----
// The value of colour id 0..8 in channel ch (ids 0..7 packed a byte each; id 8 is (35, 35, 35)).
template <int DEPTH>
__host__ __device__ __forceinline__ uint32_t tetris_shade(uint32_t id, int ch) {
  const uint64_t pk = DEPTH == 1 ? 0xBEAB5BA47FA08800ULL
                                 : (ch == 0 ? 0x969232FF7864FF00ULL : (ch == 1 ? 0xA1CA788C6CC85500ULL : 0xDA493432F5735500ULL));
  return id >= 8u ? 35u : (uint32_t)(pk >> (8 * id)) & 0xffu;
}
__host__ __device__ __forceinline__ uint32_t tetris_background(int cx, int cy) {
  return (cx < kTetrisCols && ((cx ^ cy) & 1) == 0) ? 8u : 0u;
}
// The colour id of cell (cx in 0..15, cy in 0..21) in a snapshot.
__host__ __device__ __forceinline__ uint32_t tetris_cell(const uint32_t *sn, int cx, int cy) {
  uint32_t c = tetris_background(cx, cy);
  if (cx < kTetrisCols) {
    const uint32_t b = (sn[cy] >> (3 * cx)) & 7u;
    if (b != 0u) c = b;
  }
  const uint32_t pk = sn[22], masks = sn[23];  // piece | x << 4 | y << 8 | next << 16; the two bit matrices
  int dx = cx - (int)((pk >> 4) & 0xfu), dy = cy - (int)((pk >> 8) & 0x1fu);
  if ((unsigned)dx < 4u && (unsigned)dy < 4u && ((masks >> (4 * dy + dx)) & 1u) != 0u) c = pk & 0xfu;
  dx = cx - 11;
  dy = cy - 2;
  if ((unsigned)dx < 4u && (unsigned)dy < 4u && ((masks >> (16 + 4 * dy + dx)) & 1u) != 0u) c = (pk >> 16) & 0xfu;
  return c;
}
__host__ __device__ __forceinline__ int tetris_cell_row(int i) { return (((2 * i + 1) * 33) / 14) / 18; }
__host__ __device__ __forceinline__ int tetris_cell_col(int j) { return (((2 * j + 1) * 12) / 7) / 18; }
// 32-bit word w of an env's stacked state = the four stack bytes (oldest in the low byte) of channel
// w % DEPTH of pixel w / DEPTH: prev's word shifted down by the pushes, the new values above it. live:
// whether the pixel's cell row is in the trace's live mask (otherwise every pushed value is background).
template <int DEPTH>
__host__ __device__ __forceinline__ uint32_t tetris_word(int w, uint32_t prev_word, const TetrisTrace &tr, bool live) {
  const int pix = w / DEPTH, ch = w - pix * DEPTH;
  const int i = pix / 84, j = pix - i * 84;
  const int cx = tetris_cell_col(j), cy = tetris_cell_row(i);
  const int count = tr.count, base = tr.pushes - count;
  uint32_t v = count < 4 ? prev_word >> (8 * count) : 0u;
  if (!live) {
    const uint32_t rep = count >= 4 ? 0x01010101u : (count <= 0 ? 0u : 0x01010101u << (8 * (4 - count)));
    return v | tetris_shade<DEPTH>(tetris_background(cx, cy), ch) * rep;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < count) v |= tetris_shade<DEPTH>(tetris_cell(tr.snap[(base + k) & 3], cx, cy), ch) << (8 * (4 - count + k));
  return v;
}
__host__ __device__ __forceinline__ bool tetris_row_live(const TetrisTrace &tr, int i) {
  return ((tr.live >> tetris_cell_row(i)) & 1u) != 0u;
}

}  // namespace mt
