// Heads and loss of the policy/value network on gfx950: the heads forward (A7, with the rollout's
// draw), the loss + head backward (A10, with the optional n-step scan) and the head weight gradient.
//
// Reference: policy_v_network.py:19-74 (heads + loss). The small heads (critic 1, actor A,
// repetition R outputs) and the loss are one workgroup per row.
#pragma once
#include "arch.h"

namespace mt {

struct HeadParams {
  const float *Wc, *bc, *Wa, *ba, *Wr, *br;
  int A, R, F;
  int nq;  // f32x4 quads of the head region [Wc, end of the parameters): critic | actor | repetition
};

// The three head (weights, biases) pairs are the last variables of every layout (add_heads), each
// 64-float aligned, so [Wc, P + nparams) is one contiguous 256-B-aligned region.
static HeadParams head_params(const mt_net *n, const float *P) {
  HeadParams h;
  h.F = n->F;
  h.A = n->cfg.num_actions;
  h.R = n->cfg.num_reps;
  h.Wc = P + n->off_critic;
  h.bc = h.Wc + h.F;
  h.Wa = P + n->off_actor;
  h.ba = h.Wa + (size_t)h.F * h.A;
  h.Wr = P + n->off_rep;
  h.br = h.Wr + (size_t)h.F * h.R;
  h.nq = (int)((n->nparams - n->off_critic) / 4);
  return h;
}

// Head output o (0 = critic, 1..A = actor, 1+A.. = repetition) inside the head region staged in
// LDS (heads_row): offset of its weight for feature 0, the feature stride, and its bias.
__device__ __forceinline__ void head_col_lds(const HeadParams &hp, int o, int &base, int &stride, int &bias) {
  // selects only (no branches): o is wave-uniform, so these are a few scalar instructions
  const int oa = (int)(hp.Wa - hp.Wc), orr = (int)(hp.Wr - hp.Wc);
  const bool c = o == 0, a = o <= hp.A;
  const int k = a ? o - 1 : o - 1 - hp.A;  // column within the actor / repetition block
  const int w0 = a ? oa : orr, st = a ? hp.A : hp.R;
  base = c ? 0 : w0 + k;
  stride = c ? 1 : st;
  bias = c ? hp.F : w0 + hp.F * st + k;
}

// Softmax over n logits held in lanes [0, n) of one wave (x/temp, TF: exp(x-max)/sum).
__device__ __forceinline__ float wave_softmax(float x, int lane, int n) {
  const float xm = lane < n ? x : -INFINITY;
  const float mx = wave_max(xm);
  const float e = lane < n ? expf(x - mx) : 0.f;
  const float s = wave_sum(e);
  return e / s;
}

constexpr int kMaxHeads = 64;  // 1 + A + R <= 64
constexpr int kMaxScan = 1024;  // max t_max of the fused n-step scan (mt_returns_loss_backward)
// Dynamic LDS the heads and loss kernels may ask for: the largest head region mt_net_create accepts
// (F = 512, A = 32, R = 31: 64 outputs x 513 rows, each (w, b) pair 64-float aligned = 131,840 bytes).
// With loss_bwd_kernel's ~10.5 KB of static LDS (the scan buffer, the bootstrap's features) that stays
// inside the 160 KB of a CU; a cap of 150 KB did not, and hipFuncSetAttribute refused it (invalid
// argument), so no head region above 64 KB could run the loss kernel.
constexpr size_t kHeadRegionMaxBytes = 132 * 1024;

// draw_index (common.h) over probabilities held in lanes [0, n): same order and rounding.
__device__ __forceinline__ int wave_draw(float p, int n, double u) {
  const double epsneg = 5.9604644775390625e-08;
  double cum = 0.0;
  int res = n - 1;
  for (int j = 0; j < n - 1; ++j) {
    const float pj = lane_f(p, j);  // (j is wave-uniform: a readlane, not an LDS-routed shuffle)
    cum += (double)(pj - (float)epsneg);
    if (res == n - 1 && u < cum) res = j;
  }
  return res;
}
// choose_index (common.h) over probabilities held in lanes [0, n): the e-greedy / argmax chooser. The
// first-maximum search walks n readlanes, as wave_draw does: values and the running best are
// wave-uniform, so the walk is scalar compares and selects.
__device__ __forceinline__ int wave_choose(float p, int n, double u, double eps) {
  float bv = lane_f(p, 0);
  int best = 0;
  for (int j = 1; j < n; ++j) {
    const float pj = lane_f(p, j);
    if (argmax_takes(bv, pj)) {
      best = j;
      bv = pj;
    }
  }
  return u < eps ? explore_index(n, u, eps) : best;
}

// One workgroup per row b (NT / 64 waves: 4 for F <= 256, 8 for F <= 512):
//  1. h = act(sum_z slabs[z][b] + b_fc) — the split-K dense layer finished here
//     (networks.py:57-70); every thread owns F/NT features;
//  2. logits_o = [h, 1] . W_o for the 1+A+R head outputs (policy_v_network.py:22, :31, :47):
//     wave w takes outputs o = w, w + NW, ...; lanes split F and reduce with DPP;
//  3. wave 0: v = logit_0, pi = softmax(logits_A / temp), rep = softmax(logits_R / temp);
//  4. rollout path (smp.counters != null): wave 0 draws (a, r) for the row (A3, common.h).
// Latency is everything here (32 blocks at E = 32, on the macro-step's critical chain), so every
// global load is issued at the start, in the order it is needed — vmcnt retires loads in issue
// order, so a wait for the first ones never waits for the later: the draw counter, then the slab
// partials, then the dense bias, then the whole head region (every output's weights and bias) as
// coalesced 16-B loads, staged into LDS beside h — and the row's uniforms are hashed from the
// counter while the slabs are in flight. (Round 4: each wave used to load its outputs' weight
// columns straight from HBM, lane f reading W[f][o] at a stride of A or R floats: one wave
// instruction touched 16-40 cache lines, ~5,600 line requests per block for NATURE's 15 outputs
// against ~500 for the region; the GEMV phase of the NATURE heads took 1.9 us.)
constexpr int kHeadQ = 8;  // region quads per thread held in registers from the kernel start
__device__ uint64_t g_zero_u64 = 0;  // read in place of an absent draw counter / sequence base

template <int FT, int SB, int NT, bool POL>
__device__ __forceinline__ void heads_row(int b, const float *__restrict__ slabs, int S, int B,
                                          const float *__restrict__ fc_b, int act, float alpha, const HeadParams &hp,
                                          float temp, float *__restrict__ H, float *__restrict__ v,
                                          float *__restrict__ pi, float *__restrict__ rep, const SampleArgs &smp,
                                          float *Ws) {
  __shared__ float hs[NT * FT];
  __shared__ float zs[64];
  const int F = hp.F, O = 1 + hp.A + hp.R;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int FMAX = NT * FT / 64;  // feature terms per lane of a column walk
  constexpr int NW = NT / 64;
  // every load below is unconditional (clamped addresses, zeros by select): a guarded load would
  // end its basic block with a wait for it
  // (1) the draw counter and the sequence base (the uniforms need them first)
  const uint64_t cnt = *(smp.counters ? smp.counters + b : &g_zero_u64);
  const uint32_t seq_base = *(smp.seq_base ? smp.seq_base : reinterpret_cast<const uint32_t *>(&g_zero_u64));
  // (2) the slab partials of the thread's features (S = 9 for the NIPS trunk: one batch)
  const size_t zs_stride = (size_t)B * F;
  float t[FT][SB];
#pragma unroll
  for (int fi = 0; fi < FT; ++fi) {
    const float *p = slabs + (size_t)b * F + min((int)threadIdx.x + NT * fi, F - 1);
#pragma unroll
    for (int u = 0; u < SB; ++u) t[fi][u] = p[(size_t)min(u, S - 1) * zs_stride];
  }
  // (3) dense bias, then the head region's first KQ * NT quads (F > 256 on 512 threads: 6, so the
  // whole region of an A = 18, R = 1 head set (Seaquest, 2,593 quads) is requested here — the
  // remainder loop below was a second global round trip, ~0.5 us)
  constexpr int KQ = NT == 512 ? 6 : kHeadQ;
  float fb[FT];
#pragma unroll
  for (int fi = 0; fi < FT; ++fi) fb[fi] = fc_b[min((int)threadIdx.x + NT * fi, F - 1)];
  const f32x4 *hsrc = reinterpret_cast<const f32x4 *>(hp.Wc);
  f32x4 wq[KQ];
#pragma unroll
  for (int q = 0; q < KQ; ++q) wq[q] = hsrc[min((int)threadIdx.x + NT * q, hp.nq - 1)];
  if (smp.advance && b == 0 && threadIdx.x == 0) {  // the replayed rollout's last reader has run
    smp.advance[0] += smp.advance_by;
    smp.advance[1] += smp.advance_by;
  }
  double ua = 0.0, ur = 0.0;
  if (w == 0) row_uniforms(smp.seed, b + smp.row0, cnt, &ua, &ur);
  // POL (e-greedy / argmax draw): the call's epsilon from the same counter, in the same shadow
  double eps = 0.0;
  if (POL && w == 0) eps = policy_epsilon(smp.policy, cnt);
  // slab sum in slab order + bias + activation
#pragma unroll
  for (int fi = 0; fi < FT; ++fi) {
    const int f = threadIdx.x + NT * fi;
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < SB; ++u)
      if (u < S) acc += t[fi][u];
    for (int z = SB; z < S; ++z) acc += slabs[(size_t)b * F + min(f, F - 1) + (size_t)z * zs_stride];  // (S > SB)
    const float h = act_fwd(acc + fb[fi], act, alpha);
    if (f < F) {
      hs[f] = h;
      H[(size_t)b * F + f] = h;
    }
  }
  // the head region into LDS (the rest of a region larger than KQ * NT quads loaded here)
  f32x4 *wdst = reinterpret_cast<f32x4 *>(Ws);
#pragma unroll
  for (int q = 0; q < KQ; ++q)
    if ((int)threadIdx.x + NT * q < hp.nq) wdst[threadIdx.x + NT * q] = wq[q];
  for (int i = threadIdx.x + NT * KQ; i < hp.nq; i += NT) wdst[i] = hsrc[i];
  __syncthreads();
  MT_PROBE_AT(2, b, 1);
  // logits: the same products and order as a column walk f = lane, lane + 64, ... then the bias.
  // (The wave index through readfirstlane and, for F a multiple of 64, a wave-uniform term count:
  // a per-lane guard made each term an exec-masked block with its own LDS round trip, and the
  // column loop a divergent one — ~0.45 us per column of a wave, probe build.)
  const int wu = __builtin_amdgcn_readfirstlane(w);
  const int jn = F >> 6;
  if ((F & 63) == 0) {
    // The wave's features read once; outputs o and o + NW per pass, every operand of both columns
    // (and their biases) requested at once. Lane offsets by 24-bit multiplies and wave-uniform term
    // offsets (j clamped to the last real term): the per-term 32-bit multiplies were quarter-rate,
    // and the bias a dependent LDS round trip after the reduction (round 6: 1.8 us for Seaquest's
    // 20 outputs, probe build).
    float hv[FMAX];
#pragma unroll
    for (int j = 0; j < FMAX; ++j) hv[j] = hs[min(lane + 64 * j, NT * FT - 1)];
    for (int o0 = wu; o0 < O; o0 += 2 * NW) {
      const int o1 = o0 + NW < O ? o0 + NW : o0;
      int b0, s0, c0, b1, s1, c1;
      head_col_lds(hp, o0, b0, s0, c0);
      head_col_lds(hp, o1, b1, s1, c1);
      const int l0 = b0 + __mul24(lane, s0), l1 = b1 + __mul24(lane, s1);
      float w0[FMAX], w1[FMAX];
#pragma unroll
      for (int j = 0; j < FMAX; ++j) {
        const int jj = min(j, jn - 1);
        w0[j] = Ws[l0 + jj * 64 * s0];
        w1[j] = Ws[l1 + jj * 64 * s1];
      }
      const float bias0 = Ws[c0], bias1 = Ws[c1];
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int j = 0; j < FMAX; ++j)
        if (j < jn) {
          a0 += hv[j] * w0[j];
          a1 += hv[j] * w1[j];
        }
      a0 = wave_sum(a0);
      a1 = wave_sum(a1);
      if (lane == 0) {
        zs[o0] = a0 + bias0;
        if (o1 != o0) zs[o1] = a1 + bias1;
      }
    }
  } else {
    for (int o = wu; o < O; o += NW) {
      int base, stride, bias;
      head_col_lds(hp, o, base, stride, bias);
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < FMAX; ++j)
        if (lane + 64 * j < F) acc += hs[lane + 64 * j] * Ws[base + (lane + 64 * j) * stride];
      acc = wave_sum(acc);
      if (lane == 0) zs[o] = acc + Ws[bias];
    }
  }
  __syncthreads();
  MT_PROBE_AT(2, b, 2);
  if (w != 0) return;
  const float z = lane < O ? zs[lane] : 0.f;
  if (lane == 0) v[b] = z;
  // actor logits sit in lanes 1..A, repetition logits in lanes 1+A..A+R: shift them to 0..
  // (wave-uniform shortcuts with identical results for finite logits: x / 1 = x, and a one-way
  // softmax is exp(0) / 1 = 1 — the two IEEE divisions and the whole repetition softmax were a
  // third of this single wave's instructions for the non-FiGAR heads)
  float za = __shfl(z, (lane + 1) & 63, 64);
  float zr = __shfl(z, (lane + 1 + hp.A) & 63, 64);
  if (temp != 1.f) {
    za = za / temp;
    zr = zr / temp;
  }
  const float pa = wave_softmax(za, lane, hp.A);
  const float pr = hp.R == 1 ? (lane == 0 ? 1.f : 0.f) : wave_softmax(zr, lane, hp.R);
  if (lane < hp.A) pi[(size_t)b * hp.A + lane] = pa;
  if (lane < hp.R) rep[(size_t)b * hp.R + lane] = pr;
  if (smp.counters) {
    const int a = POL ? wave_choose(pa, hp.A, ua, eps) : wave_draw(pa, hp.A, ua);
    const int r = POL ? wave_choose(pr, hp.R, ur, eps) : wave_draw(pr, hp.R, ur);
    if (lane == 0) {
      const uint32_t seq = seq_base + smp.seq;  // (graph replay: device base)
      if (smp.packed) {  // tagged pair, one 8-byte store, no fence (SampleArgs::packed)
        const uint64_t tag = (uint64_t)(seq & 0xffffu) << 16;
        const uint64_t word = ((tag | (uint32_t)r) << 32) | tag | (uint32_t)a;
        __hip_atomic_store(smp.packed + b, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      } else if (smp.pair) {
        smp.pair[b] = a;
        smp.pair[B + b] = r;
      }
      smp.counters[b] = cnt + 1;
      smp.a_idx[b] = a;
      smp.r_idx[b] = r;
      if (smp.ready && !smp.packed) {  // release: the pair stores are visible to the host before the flag
        __threadfence_system();
        __hip_atomic_store(smp.ready + b, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

// POL: the draw's exploration policy is e-greedy or argmax (SampleArgs::policy). A template parameter,
// not a run-time branch: the multinomial kernel (POL = false) is instruction for instruction the one
// it was before the policy modes, on the single wave that ends every macro-step's chain.
template <int FT, int SB, int NT, bool POL>
__global__ __launch_bounds__(NT) void heads_fwd_kernel(const float *__restrict__ slabs, int S, int B,
                                                        const float *__restrict__ fc_b, int act,
                                                        float alpha, HeadParams hp, float temp,
                                                        float *__restrict__ H, float *__restrict__ v,
                                                        float *__restrict__ pi,
                                                        float *__restrict__ rep, SampleArgs smp) {
  extern __shared__ __attribute__((aligned(16))) float head_region[];
  MT_PROBE_AT(2, blockIdx.x, 0);
  heads_row<FT, SB, NT, POL>(blockIdx.x, slabs, S, B, fc_b, act, alpha, hp, temp, H, v, pi, rep, smp, head_region);
  MT_PROBE_AT(2, blockIdx.x, 3);
}

// heads_fwd_kernel for F features (<= 512) and S slabs: one feature per thread (256 threads for
// F <= 256, 512 above: the GEMV is instruction-issue bound with one wave per SIMD, so 8 waves take
// fewer output passes each — round 6) and SB >= S slabs in registers (else one batch of 16).
static int launch_heads(int rows, hipStream_t s, const float *slabs, int S, int B, const float *fc_b, int act,
                        float alpha, const HeadParams &hp, float temp, float *H, float *v, float *pi, float *rep,
                        const SampleArgs &smp) {
  if (hp.F > 512 || 1 + hp.A + hp.R > kMaxHeads) {
    set_error("heads: F = %d > 512 or %d outputs > %d", hp.F, 1 + hp.A + hp.R, kMaxHeads);
    return MT_ERR_ARG;
  }
  // dynamic LDS: the head region (<= 64 outputs x 513 rows: 132 KB at most)
  const size_t lds = (size_t)hp.nq * 16;
  if (lds > kHeadRegionMaxBytes) {
    set_error("heads: head region of %zu bytes exceeds the LDS", lds);
    return MT_ERR_ARG;
  }
#define MT_HEADS_(FT_, SB_, NT_, POL_)                                                                       \
  do {                                                                                                       \
    static bool attr_set = false;                                                                            \
    if (!attr_set && lds > 64 * 1024) {                                                                      \
      MT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&heads_fwd_kernel<FT_, SB_, NT_, POL_>),     \
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHeadRegionMaxBytes));  \
      attr_set = true;                                                                                       \
    }                                                                                                        \
    hipLaunchKernelGGL((heads_fwd_kernel<FT_, SB_, NT_, POL_>), dim3(rows), dim3(NT_), lds, s, slabs, S, B,    \
                       fc_b, act, alpha, hp, temp, H, v, pi, rep, smp);                                      \
  } while (0)
#define MT_HEADS(FT_, SB_, NT_)                                                 \
  do {                                                                          \
    if (smp.counters && smp.policy.mode != MT_POLICY_MULTINOMIAL)               \
      MT_HEADS_(FT_, SB_, NT_, true);                                           \
    else                                                                        \
      MT_HEADS_(FT_, SB_, NT_, false);                                          \
  } while (0)
  if (hp.F <= 256) {
    if (S <= 1) MT_HEADS(1, 1, 256);
    else if (S <= 9) MT_HEADS(1, 9, 256);
    else MT_HEADS(1, 16, 256);
  } else {
    if (S <= 1) MT_HEADS(1, 1, 512);
    else if (S <= 9) MT_HEADS(1, 9, 512);
    else MT_HEADS(1, 16, 512);
  }
#undef MT_HEADS
#undef MT_HEADS_
  MT_LAUNCHED();
  return MT_OK;
}

// dL/dlogit for one softmax head (policy_v_network.py:29-57, :59-74), one wave, lanes [0, n):
// objective = adv*log(p_sel + 1e-30) + beta*H,  H = -sum p*log(p + 1e-30),  L = -scale*objective.
// Chain rule exactly as TF differentiates it: g_k = dL/dp_k, dz_k = p_k (g_k - sum_j p_j g_j),
// dlogit_k = dz_k / temp. Returns lane's dlogit; *ent, *lsel receive H and log(p_sel+eps).
__device__ __forceinline__ float head_softmax_grad(float p, int lane, int n, int sel, float adv,
                                                   float beta, float scale, float temp, float *ent,
                                                   float *lsel) {
  const float eps = 1e-30f;
  const bool on = lane < n;
  const float pe = p + eps;
  const float lp = on ? logf(pe) : 0.f;
  const float e = wave_sum(on ? -(p * lp) : 0.f);
  *ent = e;
  *lsel = __shfl(lp, sel, 64);
  // d objective / dp_k = adv*[k==sel]/(p+eps) + beta * d(-sum p log(p+eps))/dp_k
  //                    = adv*[k==sel]/(p+eps) - beta*(log(p+eps) + p/(p+eps))
  float dobj = on ? ((lane == sel ? adv / pe : 0.f) - beta * (lp + p / pe)) : 0.f;
  const float g = -scale * dobj;
  const float sg = wave_sum(on ? p * g : 0.f);
  return on ? p * (g - sg) / temp : 0.f;
}

// One workgroup per row b: head gradients dz[b][0..O) and dH[b][f] = act'(H) * sum_o dz_o W[f][o].
// Optional n-step scan inside the loss kernel (mt_returns_loss_backward): row b = t*E + e.
struct ReturnsSrc {
  const float *r = nullptr, *mask = nullptr, *VT = nullptr;  // r / mask [T][E] (host-mapped ok)
  double gamma = 0.0;
  int T = 0, E = 0;
  float *y_out = nullptr, *adv_out = nullptr;
  // bootstrap from the rollout's last chain without its heads kernel (mt_returns_loss_backward_boot):
  // V(s_T)[e] = [act(sum_z boot_slabs[z][e] + fc_b), 1] . [Wc, bc] computed by the loss block
  // itself (VT unused), written to vt_out[e] by the blocks of step 0
  const float *boot_slabs = nullptr, *fc_b = nullptr;
  int boot_S = 0;
  float *vt_out = nullptr;
  // BAYESIAN (mt_dropout_returns_loss_backward, the kernel's RV variant): the rollout's values [T][E].
  // adv = R - v_roll[b], while the critic term and loss_terms keep the kernel's `v` (the redrawn v')
  const float *v_roll = nullptr;
};

// V(s_T)[e] of the bootstrap (ReturnsSrc::boot_slabs): the dense layer's split-K slabs summed in
// slab order + bias + act (heads_row's phase 1), then the critic's dot product as heads_row forms
// it (lanes over features in 64-strides, DPP wave sum, + bias) from the head region in LDS (Ws).
// Called by the whole block; the result is in *vt (LDS) after the call. stage(): the caller's LDS
// stores of the head region, run after this block's slab loads are issued and before the barrier.
template <class Pre, class Stage>
__device__ __forceinline__ void boot_value(const ReturnsSrc &rs, const HeadParams &hp, int e, int act, float alpha,
                                           const float *Ws, float *hsb, float *vt, const Pre &pre, const Stage &stage) {
  const int F = hp.F;
  const size_t zs_stride = (size_t)rs.E * F;
  if (F <= 512 && rs.boot_S <= 16) {
    // every slab partial and dense bias of the thread's features requested first, THEN pre() (the
    // caller's pinned-memory reward loads): vector loads retire in issue order, so a PCIe load
    // issued ahead of these made the slab sum wait for it (round 5)
    float t[2][16], fb[2];
#pragma unroll
    for (int fi = 0; fi < 2; ++fi) {
      const int fc = min((int)threadIdx.x + 256 * fi, F - 1);
      const float *p = rs.boot_slabs + (size_t)e * F + fc;
#pragma unroll
      for (int u = 0; u < 16; ++u) t[fi][u] = p[(size_t)min(u, rs.boot_S - 1) * zs_stride];
      fb[fi] = rs.fc_b[fc];
    }
    pre();
#pragma unroll
    for (int fi = 0; fi < 2; ++fi) {
      const int f = threadIdx.x + 256 * fi;
      if (f < F) {
        float acc = 0.f;
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (u < rs.boot_S) acc += t[fi][u];
        hsb[f] = act_fwd(acc + fb[fi], act, alpha);
      }
    }
  } else {
    pre();
    for (int f = threadIdx.x; f < F; f += 256) {
      const float *p = rs.boot_slabs + (size_t)e * F + f;
      float acc = 0.f;
      for (int z = 0; z < rs.boot_S; z += 16) {
        float t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) t[u] = p[(size_t)min(z + u, rs.boot_S - 1) * zs_stride];
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (z + u < rs.boot_S) acc += t[u];
      }
      hsb[f] = act_fwd(acc + rs.fc_b[f], act, alpha);
    }
  }
  stage();
  __syncthreads();
  if (threadIdx.x < 64) {  // heads_row's critic column: same products, same order
    const int lane = threadIdx.x;
    float acc = 0.f;
    if ((F & 63) == 0) {
      const int jn = F >> 6;
      float hv[8], wv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        hv[j] = hsb[min(lane + 64 * j, 511)];
        wv[j] = Ws[min(lane + 64 * j, F - 1)];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < jn) acc += hv[j] * wv[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (lane + 64 * j < F) acc += hsb[lane + 64 * j] * Ws[lane + 64 * j];
    }
    acc = wave_sum(acc);
    if (lane == 0) *vt = acc + Ws[F];
  }
  __syncthreads();
}

// returns_kernel's arithmetic for row b = (t, e): R from T-1 down to t, bit-identical to
// mt_returns. Thread k < 256 brings step t + k's reward / mask in (rk, mk: requested by the caller
// before its other work, one round trip), the rest load here; thread 0 scans (vb = V[b], which it
// loaded with the head inputs). Called by the whole block.
__device__ __forceinline__ void row_return(const ReturnsSrc &rs, float vb, int b, float vt,
                                           float rk, float mk, float *ya, float *buf) {
#pragma clang fp contract(off)
  const int T = rs.T, E = rs.E;
  const int t = b / E, e = b - t * E, n = T - t;  // steps t .. T-1
  if ((int)threadIdx.x < n) {
    buf[2 * threadIdx.x] = rk;
    buf[2 * threadIdx.x + 1] = mk;
  }
  for (int k = threadIdx.x + 256; k < n; k += 256) {
    buf[2 * k] = rs.r[(size_t)(t + k) * E + e];
    buf[2 * k + 1] = rs.mask[(size_t)(t + k) * E + e];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float g32 = __fmul_rn((float)rs.gamma, vt);
    double R = (double)buf[2 * (n - 1)] + (double)g32 * (double)buf[2 * (n - 1) + 1];
    const double gd = rs.gamma;
    for (int k = n - 2; k >= 0; --k) R = (double)buf[2 * k] + (gd * R) * (double)buf[2 * k + 1];
    ya[0] = (float)R;
    ya[1] = (float)(R - (double)vb);
    rs.y_out[b] = ya[0];
    rs.adv_out[b] = ya[1];
  }
  __syncthreads();
}

// RV (compile-time, BAYESIAN's fused update): the advantage's value is rs.v_roll[b], loaded with the
// row's other head inputs ahead of the scan; RV = false is the kernel of every other arch, unchanged.
template <bool RV>
__global__ __launch_bounds__(256) void loss_bwd_kernel(
    HeadParams hp, const float *__restrict__ H, const float *__restrict__ pi,
    const float *__restrict__ rep, const float *__restrict__ v, const int32_t *__restrict__ a_idx,
    const int32_t *__restrict__ r_idx, const float *__restrict__ y, const float *__restrict__ adv,
    float beta, float scale, float temp, int act, float alpha, float *__restrict__ dz,
    float *__restrict__ dH, float *__restrict__ loss_terms, ReturnsSrc rs) {
  __shared__ float dzs[kMaxHeads];
  __shared__ float ya[2];
  __shared__ float buf[2 * kMaxScan];
  extern __shared__ __attribute__((aligned(16))) float Ws[];  // the head region (HeadParams::nq quads)
  const int b = blockIdx.x;
  MT_PROBE_AT(4, b, 0);
  const int A = hp.A, R = hp.R, O = 1 + A + R, F = hp.F;
  // Every load that does not depend on the return is issued first, so its latency overlaps the
  // scan's (the rewards / masks are read over PCIe from pinned memory): the row's head inputs
  // (threads < 64), H[b][f] of the thread's features and the head region as coalesced 16-B loads
  // (staged into LDS for the critic's dot product and dH; round 4: per-thread loads of W[f][.] at a
  // stride of A or R floats made ~2,800 cache-line requests per block for NATURE's heads, queued
  // ahead of the bootstrap slab loads).
  const int lane = threadIdx.x;
  float pa = 0.f, pr = 0.f, vb = 0.f, adv_in = 0.f, y_in = 0.f;
  [[maybe_unused]] float vroll = 0.f;
  int ai = 0, ri = 0;
  if (threadIdx.x < 64) {
    pa = lane < A ? pi[(size_t)b * A + lane] : 0.f;
    pr = lane < R ? rep[(size_t)b * R + lane] : 0.f;
    vb = v[b];
    if constexpr (RV) vroll = rs.v_roll[b];
    ai = a_idx[b];
    ri = r_idx[b];
    if (!rs.r) {
      adv_in = adv[b];
      y_in = y[b];
    }
  }
  constexpr int FT = 2;  // F <= 512 in registers (more: read at the end)
  float hv[FT];
#pragma unroll
  for (int fi = 0; fi < FT; ++fi) hv[fi] = H[(size_t)b * F + min((int)threadIdx.x + 256 * fi, F - 1)];
  const f32x4 *hsrc = reinterpret_cast<const f32x4 *>(hp.Wc);
  f32x4 wq[kHeadQ];
#pragma unroll
  for (int q = 0; q < kHeadQ; ++q) wq[q] = hsrc[min((int)threadIdx.x + 256 * q, hp.nq - 1)];
  auto stage = [&]() {
    f32x4 *wdst = reinterpret_cast<f32x4 *>(Ws);
#pragma unroll
    for (int q = 0; q < kHeadQ; ++q)
      if ((int)threadIdx.x + 256 * q < hp.nq) wdst[threadIdx.x + 256 * q] = wq[q];
    for (int i = threadIdx.x + 256 * kHeadQ; i < hp.nq; i += 256) wdst[i] = hsrc[i];
  };
  bool staged = false;
  if (rs.r) {
    // this row's rewards / masks (pinned host memory, a PCIe round trip): requested right behind the
    // bootstrap slab loads (boot_value's pre), whose sum would otherwise wait for them
    float rk = 0.f, mk = 0.f;
    auto rewards = [&]() {
      const int t = b / rs.E, e = b - t * rs.E;
      if ((int)threadIdx.x < rs.T - t) {
        rk = rs.r[(size_t)(t + threadIdx.x) * rs.E + e];
        mk = rs.mask[(size_t)(t + threadIdx.x) * rs.E + e];
      }
    };
    float vt;
    if (rs.boot_slabs) {
      __shared__ float hsb[512];
      __shared__ float vts;
      const int e = b % rs.E;
      boot_value(rs, hp, e, act, alpha, Ws, hsb, &vts, rewards, stage);
      staged = true;
      vt = vts;
      if (rs.vt_out && b < rs.E && threadIdx.x == 0) rs.vt_out[e] = vt;
    } else {
      rewards();
      vt = rs.VT[b % rs.E];
    }
    MT_PROBE_AT(4, b, 1);
    row_return(rs, RV ? vroll : vb, b, vt, rk, mk, ya, buf);
  }
  MT_PROBE_AT(4, b, 2);
  if (!staged) stage();  // (visible to every thread after the barrier below)
  if (threadIdx.x < 64) {
    const float ad = rs.r ? ya[1] : adv_in;
    const float yb = rs.r ? ya[0] : y_in;
    float ent_a, ls_a, ent_r, ls_r;
    const float ga = head_softmax_grad(pa, lane, A, ai, ad, beta, scale, temp, &ent_a, &ls_a);
    const float gr = head_softmax_grad(pr, lane, R, ri, ad, beta, scale, temp, &ent_r, &ls_r);
    const float diff = yb - vb;
    // d/dv of scale * 0.25 * (y - v)^2  (policy_v_network.py:25-26)
    const float gv = scale * 0.25f * 2.0f * (vb - yb);
    if (lane == 0) dzs[0] = gv;
    if (lane < A) dzs[1 + lane] = ga;
    if (lane < R) dzs[1 + A + lane] = gr;
    if (lane == 0 && loss_terms) {
      loss_terms[(size_t)b * 4 + 0] = 0.25f * diff * diff;
      loss_terms[(size_t)b * 4 + 1] = -((ls_a + ls_r) * ad);
      loss_terms[(size_t)b * 4 + 2] = ent_a;
      loss_terms[(size_t)b * 4 + 3] = ent_r;
    }
  }
  __syncthreads();
  MT_PROBE_AT(4, b, 3);
  for (int o = threadIdx.x; o < O; o += 256) dz[(size_t)b * O + o] = dzs[o];
  // dH[b][f] = act'(H) * (dz_c Wc[f] + actor terms + repetition terms), in that order
  const int oa = (int)(hp.Wa - hp.Wc), orr = (int)(hp.Wr - hp.Wc);
  auto dh = [&](int f, float h) {
    float acc = dzs[0] * Ws[f];
    for (int k = 0; k < A; ++k) acc += dzs[1 + k] * Ws[oa + f * A + k];
    for (int k = 0; k < R; ++k) acc += dzs[1 + A + k] * Ws[orr + f * R + k];
    dH[(size_t)b * F + f] = acc * act_bwd(h, act, alpha);
  };
#pragma unroll
  for (int fi = 0; fi < FT; ++fi)
    if ((int)threadIdx.x + 256 * fi < F) dh(threadIdx.x + 256 * fi, hv[fi]);
  for (int f = threadIdx.x + 256 * FT; f < F; f += 256) dh(f, H[(size_t)b * F + f]);  // (F > 512: not built today)
  MT_PROBE_AT(4, b, 4);
}

// Head weight/bias gradient: G[f][o] = sum_b [H,1][b][f] * dz[b][o], scattered into the three
// (w, b) variable pairs of the flat gradient. Block = (64 features, output o): column o of dz is
// staged in LDS, the 4 waves take contiguous quarters of the rows (H read coalesced: consecutive
// lanes = consecutive features, 4 independent accumulators per lane), and the 4 wave partials are
// added in wave order through LDS (deterministic).
__device__ __forceinline__ void head_wgrad_body(const float *__restrict__ H, const float *__restrict__ dz, int B,
                                                int F, int A, int R, float *__restrict__ gc, float *__restrict__ ga,
                                                float *__restrict__ gr, int bx, int o, float *dzs) {
  // dzs: [B] column o, then [4][64] partials
  const int O = 1 + A + R;
  for (int i = threadIdx.x; i < B; i += 256) dzs[i] = dz[(size_t)i * O + o];
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int f = bx * 64 + lane;  // f == F is the bias row
  const int q = (B + 3) / 4, b0 = w * q, b1 = min(B, b0 + q);
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (f <= F) {
    int b = b0;
    if (f < F) {
      // 16 rows' loads in flight per trip (a 4-row trip waited out one load latency per 4 rows);
      // accumulator u still takes rows b0 + u, b0 + 4 + u, ... in order
      for (; b + 15 < b1; b += 16) {
        float h[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) h[u] = H[(size_t)(b + u) * F + f];
#pragma unroll
        for (int u = 0; u < 16; ++u) a[u & 3] += h[u] * dzs[b + u];
      }
      for (; b + 3 < b1; b += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] += H[(size_t)(b + u) * F + f] * dzs[b + u];
      }
      for (; b < b1; ++b) a[0] += H[(size_t)b * F + f] * dzs[b];
    } else {
      for (; b < b1; ++b) a[0] += dzs[b];
    }
  }
  float *part = dzs + B;
  part[w * 64 + lane] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  if (w != 0 || f > F) return;
  const float acc = ((part[lane] + part[64 + lane]) + part[128 + lane]) + part[192 + lane];
  if (o == 0)
    gc[f] = acc;  // [F][1] weights then the bias at index F
  else if (o <= A)
    ga[(size_t)f * A + (o - 1)] = acc;
  else
    gr[(size_t)f * R + (o - 1 - A)] = acc;
}

// The head weight gradient as a job of a grouped launch: block (f chunk of 64, output o).
struct HeadWgradJob {
  const float *H, *dz;
  int B, F, A, R;
  float *gc, *ga, *gr;
  __host__ __device__ int gx() const { return (F + 1 + 63) / 64; }
  __host__ __device__ int blocks() const { return gx() * (1 + A + R); }
  size_t lds() const { return sizeof(float) * ((size_t)B + 4 * 64); }
  __device__ __forceinline__ void run(int id, float *smem) const {
    head_wgrad_body(H, dz, B, F, A, R, gc, ga, gr, id % gx(), id / gx(), smem);
  }
};

}  // namespace mt
