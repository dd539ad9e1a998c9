// BAYESIAN arch (networks.py:194-204): the dropout + fc4 stage between the NIPS trunk's dense layer
// and the heads, and the epilogue of its backward.
//
//   H3 = act(sum_z slabs[z] + b3)              (the NIPS net's H, bit for bit: heads_row's arithmetic)
//   D  = tf.nn.dropout(H3, keep) = (H3 / keep) * m,  m from common.h's counter-based mask
//   Z4 = D @ W4                                (one slab; heads_fwd_kernel adds b4, activates, runs the heads)
//
// Dropout state lives in the workspace (region 7): {seed, row0, counters[rows]}. Row b's mask is keyed
// on (seed, row0 + b, counters[b]); the block that owns the row increments its counter at the end of
// the stage (the sampler's pattern), so every call — a replayed one included — draws a fresh mask.
#pragma once
#include "gemm.h"

namespace mt {

struct DropoutFcArgs {
  const float *slabs;  // fc3 split-K partials [S][B][256]; null: H3 is read, not formed (mt_dropout_redraw)
  int S, B;
  const float *fc_b;   // fc3 biases
  int act;
  float alpha;
  float *H3;           // [B][256] fc3 after bias and activation
  uint8_t *mask;       // [B][256] 0 / 1
  float *D;            // [B][256] the dropped features (the backward's fc4 weight-gradient operand)
  uint64_t *state;     // {seed, row0, counters[B]}
  const float *W4;     // [256][256] (in, out)
  float keep;
  float *Z4;           // [B][256]
};

// One block = 16 rows x all 256 output columns, so it alone owns its rows' counters. 16 waves:
//  phase 1: wave w owns row w of the tile, lane l its features 4l .. 4l+3 — exactly one 64-bit mask
//           word per lane, one counter per wave; H3, D as 16-B accesses, the mask as one 4-byte store;
//  phase 2: wave w owns output columns [16w, 16w + 16), one 16x16 accumulator, 64
//           v_mfma_f32_16x16x4_f32 over K = 256 with A = D from LDS, B = W4 held in registers.
// The launch is latency-bound (2 blocks at E = 32), so the waves are chosen for the critical path: a
// SIMD's MFMA work is the same with 4, 8 or 16 waves (256 MFMAs per SIMD; fewer waves only make one
// wave walk several tiles in series), while 16 waves put every global load of the block in flight at
// the kernel start, in the order it is needed (vector loads retire in issue order): the counter, the
// row's slab partials (up to 9: the fused trunk's), the bias, then the wave's whole W4 column tile
// (64 loads per lane, W4's 256 KB from L2), which lands under the slab sum and the mask hash.
// (Measured at E = 32, back-to-back forwards against the NIPS net's, DESIGN.md "BAYESIAN arch": a first
// form that summed the slabs in a loop of dependent loads, four rows per thread, made the stage
// 16.9 us; this one 8.5 us. Reading W4 as 16-B
// quads — four strided tiles per wave over a K quarter, the quarters added through LDS — was no
// faster, 9.4 us with 4 spilled registers: the floor is the block's 256 MFMAs per SIMD, ~3.4 us.)
// Loads are unconditional (rows >= B of a ragged last tile clamp to row B - 1, in bounds); such rows
// write nothing and their D is zero in LDS.
constexpr int kDropRows = 16;
constexpr int kDropThreads = 1024;
constexpr int kDropLd = kDropF + 4;  // LDS row stride of D (b128 fragment reads, no bank conflicts)
constexpr int kDropSB = 9;           // slab partials per batch of loads

__global__ __launch_bounds__(kDropThreads) void dropout_fc_kernel(DropoutFcArgs a) {
  __shared__ __attribute__((aligned(16))) float Ds[kDropRows * kDropLd];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int row0 = blockIdx.x * kDropRows;
  // (1a) loads of phase 1: row b = row0 + w (clamped), features c4 .. c4 + 3
  const int b = row0 + w, bc = min(b, a.B - 1), c4 = 4 * lane;
  const bool live = b < a.B, fwd = a.slabs != nullptr;
  const size_t e = (size_t)bc * kDropF + c4;
  const uint64_t seed = a.state[0], grow0 = a.state[1], cnt = a.state[2 + bc];
  const int S = fwd ? a.S : 1;  // (redraw: the one "slab" is the stored H3)
  const size_t zs4 = (size_t)a.B * kDropF / 4;
  const f32x4 *src = reinterpret_cast<const f32x4 *>((fwd ? a.slabs : a.H3) + e);
  f32x4 tt[kDropSB];
#pragma unroll
  for (int u = 0; u < kDropSB; ++u) tt[u] = src[(size_t)min(u, S - 1) * zs4];
  const f32x4 bias = *reinterpret_cast<const f32x4 *>(fwd ? a.fc_b + c4 : a.W4);
  // (1b) the wave's W4 column tile: fragment element s of chunk kc holds k = 16 kc + 4 g + s (gemm.h)
  float bf[64];
  {
    const float *wp = a.W4 + (size_t)(4 * g) * kDropF + 16 * w + r;
#pragma unroll
    for (int kc = 0; kc < 16; ++kc)
#pragma unroll
      for (int s = 0; s < 4; ++s) bf[kc * 4 + s] = wp[(size_t)(16 * kc + s) * kDropF];
  }
  // (1c) H3 = act(slabs in slab order + bias) — heads_row's arithmetic, bit for bit — mask, D
  f32x4 h = tt[0];
  if (fwd) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < kDropSB; ++u)
      if (u < S) acc += tt[u];
    for (int z0 = kDropSB; z0 < S; z0 += kDropSB) {  // (S > 9: the layered forward's split-K)
#pragma unroll
      for (int u = 0; u < kDropSB; ++u) tt[u] = src[(size_t)min(z0 + u, S - 1) * zs4];
#pragma unroll
      for (int u = 0; u < kDropSB; ++u)
        if (z0 + u < S) acc += tt[u];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = act_fwd(acc[k] + bias[k], a.act, a.alpha);
  }
  const uint64_t word = dropout_word(dropout_base(seed, grow0 + (uint64_t)bc, cnt), lane);
  f32x4 d = {0.f, 0.f, 0.f, 0.f};
  uint32_t mb = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool keep = dropout_keep(word, k, a.keep);
    // tf.nn.dropout: (x / keep_prob) * binary, an fp32 division; keep_prob == 1 returns x itself
    d[k] = a.keep == 1.f ? h[k] : __fdiv_rn(h[k], a.keep) * (keep ? 1.f : 0.f);
    mb |= (keep ? 1u : 0u) << (8 * k);
  }
  if (live) {  // (wave-uniform)
    if (fwd) *reinterpret_cast<f32x4 *>(a.H3 + e) = h;
    *reinterpret_cast<uint32_t *>(a.mask + e) = mb;
    *reinterpret_cast<f32x4 *>(a.D + e) = d;
  } else {
    d = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  *reinterpret_cast<f32x4 *>(Ds + w * kDropLd + c4) = d;
  __syncthreads();
  if (live && lane == 0) a.state[2 + b] = cnt + 1;  // the row's owner: its next call draws a fresh mask
  // (2) Z4 tile = D[16 x 256] . W4[256 x 16]
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kc = 0; kc < 16; ++kc) {
    const f32x4 av = *reinterpret_cast<const f32x4 *>(Ds + r * kDropLd + 16 * kc + 4 * g);
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bf[kc * 4 + s], acc, 0, 0, 0);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int bo = row0 + 4 * g + q;
    if (bo < a.B) a.Z4[(size_t)bo * kDropF + 16 * w + r] = acc[q];
  }
}

static int launch_dropout_fc(const DropoutFcArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(dropout_fc_kernel, dim3(cdiv(a.B, kDropRows)), dim3(kDropThreads), 0, s, a);
  MT_LAUNCHED();
  return MT_OK;
}

// dZ3 = (v * m / keep) * act'(H3), v = dZ4 . W4^T: the gradient of (x / keep) * binary, then the
// activation's, from the stored mask bytes and H3's branch (> 0 for ReLU, >= 0 for leaky, as
// EpMasked) — never from D != 0, which is also false where a kept feature is exactly zero.
struct EpDropMasked {
  float *dX;
  const float *H3;
  const uint8_t *mask;
  int ld, act;
  float alpha, keep;
  struct Pre {
    float y, m;
  };
  __device__ __forceinline__ Pre pre(int m, int n) const {
    const size_t i = (size_t)m * ld + n;
    return {H3[i], mask[i] ? 1.f : 0.f};
  }
  __device__ __forceinline__ void operator()(const Pre &p, int m, int n, int, float v) const {
    const float g = keep == 1.f ? v : __fdiv_rn(v * p.m, keep);
    dX[(size_t)m * ld + n] = g * act_bwd(p.y, act, alpha);
  }
  __device__ __forceinline__ void operator()(int m, int n, int z, float v) const { (*this)(pre(m, n), m, n, z, v); }
};

}  // namespace mt
