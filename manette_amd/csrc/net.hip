// Policy/value network of the PAAC hot path on gfx950: forward (A5-A7) and fused loss + backward
// (A10) as layer drivers over the architectures (arch.h), the heads and loss kernels (heads.h) and
// the LSTM arch (lstm.h), then the C ABI.
//
// Reference: networks.py:130-278 (trunks), policy_v_network.py:19-74 (heads + loss).
// Trunk products run on the fp32 MFMA GEMM core (gemm.h) with implicit im2col loaders.
#include "arch.h"
#include "heads.h"

namespace mt {

// ---------------------------------------------------------------------------------------------
// Layer drivers
// ---------------------------------------------------------------------------------------------
template <class G, bool U8>
static int conv_forward(const void *X, const float *Wt, const float *bias, float *Y, int B, int act,
                        float alpha, hipStream_t s) {
  using T = TileConvFwd<G>;
  LdIm2col<G, U8> la{reinterpret_cast<const typename InElem<U8>::T *>(X)};
  LdColMajor lb{Wt, G::COUT, -1};
  EpBiasAct ep{Y, bias, G::COUT, act, alpha};
  const int M = B * G::OH * G::OW;
  if constexpr (G::COUT % 32 == 0) {
    // small batches (a rollout step): a grid of under two workgroups per CU leaves most CUs idle
    // and each wave a long MFMA chain — 32 x 32 tiles, one 16 x 16 accumulator per wave
    using TS = Tile<32, 32, 2, 2, conv_bk<G::KK>()>;
    if (cdiv(M, T::BM) * cdiv(G::COUT, T::BN) < 512) return launch_gemm<TS>(la, lb, ep, M, G::COUT, G::KK, 1, s);
  }
  return launch_gemm<T>(la, lb, ep, M, G::COUT, G::KK, 1, s);
}

// Conv + bias + activation + 2x2/2 max pool in one product (pool-ordered rows, EpBiasActPool):
// Y = the pooled output, arg = the window position of each maximum.
template <class G, bool U8>
static int conv_forward_pool(const void *X, const float *Wt, const float *bias, float *Y, uint8_t *arg, int B,
                             int act, float alpha, hipStream_t s) {
  using T = TileConvFwd<G>;
  LdIm2col<G, U8, true> la{reinterpret_cast<const typename InElem<U8>::T *>(X)};
  LdColMajor lb{Wt, G::COUT, -1};
  EpBiasActPool<G> ep{Y, arg, bias, act, alpha};
  const int M = B * (G::OH / 2) * (G::OW / 2) * 4;
  if constexpr (G::COUT % 32 == 0) {
    using TS = Tile<32, 32, 2, 2, conv_bk<G::KK>()>;
    if (cdiv(M, T::BM) * cdiv(G::COUT, T::BN) < 512) return launch_gemm<TS>(la, lb, ep, M, G::COUT, G::KK, 1, s);
  }
  return launch_gemm<T>(la, lb, ep, M, G::COUT, G::KK, 1, s);
}

// dW (+db) of a conv -> grad[(KK+1) x COUT] (weights then biases): dW = im2col(X)^T . dY as a GEMM
// job into K-split slabs [S][KK+1][COUT] (one split: straight into gwb) and the slab-sum job that
// finishes it (no job when unsplit). db: when KK fills whole M-tiles (NIPS / NATURE, PWYX conv3),
// the column sums of dY per split go to slab row KK (BiasRowJob) — a 64-row MFMA tile for the one
// bias row would add a fifth of the product's work; otherwise the bias is a ones-row of the same
// GEMM (LdIm2colT), free in the last tile's spare rows.
template <class G, bool U8>
struct WgradJobs {
  PairJob<GemmJob<TileConvWgrad<G>, LdIm2colT<G, U8>, LdColMajor, EpSlab>, BiasRowJob<G::COUT>> gemm;
  SlabJob sum;
};
template <class G, bool U8>
static WgradJobs<G, U8> conv_wgrad_jobs(const void *X, const float *dY, float *slab, float *gwb, int B) {
  using T = TileConvWgrad<G>;
  const int M = G::KK + 1, K = B * G::OH * G::OW;
  const int S = conv_wgrad_splits<G>(B);
  LdIm2colT<G, U8> la{reinterpret_cast<const typename InElem<U8>::T *>(X)};
  LdColMajor lb{dY, G::COUT, -1};
  float *dst = S == 1 ? gwb : slab;
  constexpr bool sep = G::KK % T::BM == 0;
  const auto g = gemm_job<T>(la, lb, EpSlab{dst, M, G::COUT}, sep ? G::KK : M, G::COUT, K, S);
  const BiasRowJob<G::COUT> bias{dY, dst + (size_t)G::KK * G::COUT, (size_t)M * G::COUT, K, g.kchunk,
                                 sep ? g.gz : 0};
  WgradJobs<G, U8> j{{g, bias}, SlabJob{}};
  if (g.gz > 1) j.sum = SlabJob{slab, g.gz, (size_t)M * G::COUT, gwb};
  return j;
}

// The weight-gradient jobs of conv layer G: the direct kernel for the stride-1 SAME layers
// (DWgradJob, dconv.h), the generic GEMM otherwise; same slab layout and SlabJob either way.
template <class G, bool U8>
struct DWgradJobs {
  DWJobFor<G, U8> gemm;
  SlabJob sum;
};
template <class G, bool U8>
static auto conv_wgrad_jobs_sel(const void *X, const float *dY, float *slab, float *gwb, int B) {
  if constexpr (dconv_wgrad<G>()) {
    using J = DWJobFor<G, U8>;
    const int S = dwgrad_splits<G, U8>(B);
    return DWgradJobs<G, U8>{J{reinterpret_cast<const typename J::InT *>(X), dY, slab, B, S},
                             SlabJob{slab, B > 0 ? S : 0, J::D::SLAB, gwb}};
  } else {
    return conv_wgrad_jobs<G, U8>(X, dY, slab, gwb, B);
  }
}

// dX of a conv (transposed-conv gather), masked by the activation derivative of X, as a GEMM job.
template <class G>
static auto conv_dgrad_job(const float *dY, const float *Wt, const float *Xact, float *dX, int B, int act,
                           float alpha) {
  using T = TileConvDgrad<G>;
  if constexpr (PhaseGeom<G>::OK) {  // stride phases: K / (S*S), no multiplications by holes
    constexpr int S2 = G::S * G::S;
    const int mp = cdiv(B * PhaseGeom<G>::HQ * PhaseGeom<G>::WQ, T::BM) * T::BM;
    return gemm_job<T>(LdConvBwdAPhase<G>{dY, mp, B}, LdConvBwdBPhase<G>{Wt, mp / T::BM},
                       EpMaskedPhase<G>{dX, Xact, mp, B, act, alpha}, S2 * mp, G::CIN, PhaseGeom<G>::KP, 1);
  } else {
    return gemm_job<T>(LdConvBwdA<G>{dY}, LdConvBwdB<G>{Wt}, EpMasked{dX, Xact, G::CIN, act, alpha},
                       B * G::H * G::W, G::CIN, G::KH * G::KW * G::COUT, 1);
  }
}

// dX of a stride-1 conv whose input is the pooled output of conv GJ: the MaxPoolGrad routing and
// the activation mask run in the epilogue (EpMaskedUnpool), straight into GJ's full-res gradient.
template <class G, class GJ>
static auto conv_dgrad_unpool_job(const float *dY, const float *Wt, const float *Pj, const uint8_t *argj,
                                  float *dactj, int B, int act, float alpha) {
  using T = TileConvDgrad<G>;
  static_assert(!PhaseGeom<G>::OK, "pooled inputs feed stride-1 convs (networks.py:206-225)");
  return gemm_job<T>(LdConvBwdA<G>{dY}, LdConvBwdB<G>{Wt}, EpMaskedUnpool<GJ>{dactj, Pj, argj, act, alpha},
                     B * G::H * G::W, G::CIN, G::KH * G::KW * G::COUT, 1);
}

#define MT_TRY(x)              \
  do {                         \
    int rc_ = (x);             \
    if (rc_ != MT_OK) return rc_; \
  } while (0)

template <class Ar, int I>
static const float *layer_out(float *ws, const WsLayout &L) {
  return ws + (pooled<Ar, I>() ? L.pool[I] : L.act[I]);
}

// The layered trunk with the rollout chain's extras: st = the stacking source of conv1 (x = st->out;
// the NATURE gray chain: nature_chain_kernel; the frame trunks: stack_conv1_kernel, then conv2 ..
// layered), sync = the counters it uses (zero between launches).
struct FwdExtras {
  const StackSrc *st = nullptr;
  uint32_t *sync = nullptr;
};

template <class Ar, int I = 0>
static int trunk_forward(const mt_net *n, const float *P, const void *x, int B, float *ws,
                         const WsLayout &L, hipStream_t s, const FwdExtras &ex = FwdExtras{}) {
  if constexpr (I < Ar::NCONV) {
    using G = LayerG<Ar, I>;
    const float *W = P + n->off_conv[I];
    if (I == 0 && ex.st && !nature_stacking<Ar>() && !frame_stacking<Ar>()) {
      set_error("the stacking conv1 is built for the NIPS, the gray NATURE and the frame (PWYX / LSTM) trunks");
      return MT_ERR_UNSUPPORTED;
    }
    if constexpr (I == 0 && frame_stacking<Ar>()) {
      if (ex.st) {  // the rollout step: pull + stack + conv1 as one dataflow launch, then conv2 ..
        if (!ex.sync || x != ex.st->out) {
          set_error("stacking conv1: the input must be the new state rows, with a counter region");
          return MT_ERR_ARG;
        }
        MT_TRY((launch_stack_conv1<G>(*ex.st, W, ws + L.pool[0], (uint8_t *)(ws + L.parg[0]), B, n->cfg.activation,
                                      n->cfg.alpha_leaky, ex.sync, s)));
        return trunk_forward<Ar, 1>(n, P, layer_out<Ar, 0>(ws, L), B, ws, L, s);
      }
    }
    if constexpr (I == 0 && nature_stacking<Ar>()) {
      if (ex.st) {  // the rollout chain: stacking conv1 -> conv2 -> conv3 as one dataflow launch
        if (!ex.sync) {
          set_error("nature chain: no counter region");
          return MT_ERR_ARG;
        }
        return launch_nature_chain<LayerG<Ar, 0>, LayerG<Ar, 1>, LayerG<Ar, 2>>(
            *ex.st, W, P + n->off_conv[1], P + n->off_conv[2], ws + L.act[0], ws + L.act[1], ws + L.act[2], B,
            n->cfg.activation, n->cfg.alpha_leaky, ex.sync, s);
      }
    }
    // PWYX / LSTM frame trunk (stride-1 SAME) and NATURE (strided VALID): direct conv, patch in LDS (dconv.h)
    // (the RGB NATURE conv1's 768-deep K with its 24-row patch exceeds the LDS: generic)
    if constexpr ((G::S == 1 && G::SAME) || (Ar::NCONV == 3 && !G::SAME && G::CIN != 12))
      MT_TRY((conv_forward_direct<G, I == 0, pooled<Ar, I>()>(
          x, W, W + G::KK * G::COUT, ws + (pooled<Ar, I>() ? L.pool[I] : L.act[I]),
          pooled<Ar, I>() ? (uint8_t *)(ws + L.parg[I]) : nullptr, B, n->cfg.activation, n->cfg.alpha_leaky, s)));
    else if constexpr (pooled<Ar, I>())
      MT_TRY((conv_forward_pool<G, I == 0>(x, W, W + G::KK * G::COUT, ws + L.pool[I], (uint8_t *)(ws + L.parg[I]), B,
                                           n->cfg.activation, n->cfg.alpha_leaky, s)));
    else
      MT_TRY((conv_forward<G, I == 0>(x, W, W + G::KK * G::COUT, ws + L.act[I], B, n->cfg.activation,
                                      n->cfg.alpha_leaky, s)));
    return trunk_forward<Ar, I + 1>(n, P, layer_out<Ar, I>(ws, L), B, ws, L, s, ex);
  }
  return MT_OK;
}

// Conv layers I .. 0 of the backward, top down: one grouped launch per layer — its dX (the
// critical path, first), its dW GEMM and `pending` (the slab sum of layer I+1's dW) — then
// conv1's slab sum. Layer I's slabs live in region I % 2 (wslab / wslab2), so the slab sum of
// layer I+1 reads the other region while layer I's dW GEMM writes its own. `extra` (the LSTM's
// small cell / fc6 weight gradients: a few blocks, each a serial K walk) leads the top layer's
// grid, so its blocks start before the wide products fill the CUs instead of trailing them.
// Optional global-norm partials of the whole gradient written by the backward's last launch
// (world == 1: no all-reduce between the backward and the clip, so mt_grad_sumsq is not needed).
struct NormOut {
  float *partials = nullptr;  // [MT_NORM_PARTIALS]
  size_t n = 0;               // gradient floats
  NormOut() = default;
  NormOut(float *partials_, const mt_net *net) : partials(partials_), n(net->nparams) {}
};

template <class Ar, int I, class X = NoJob>
static int trunk_backward(const mt_net *n, const float *P, const uint8_t *obs, int B, float *ws,
                          const WsLayout &L, float *grad, hipStream_t s, SlabJob pending = SlabJob{},
                          const NormOut &no = NormOut{}, const X &extra = X{}) {
  using G = LayerG<Ar, I>;
  const int act = n->cfg.activation;
  const float al = n->cfg.alpha_leaky;
  const void *x = I == 0 ? (const void *)obs : (const void *)layer_out<Ar, (I > 0 ? I - 1 : 0)>(ws, L);
  if ((size_t)B * G::H * G::W * G::CIN >= ((size_t)1 << 31)) {  // LdIm2colT's 32-bit pixel offsets
    set_error("batch %d too large for the conv %d weight gradient", B, I);
    return MT_ERR_ARG;
  }
  if ((size_t)B * G::OH * G::OW * G::COUT * 4 >= ((size_t)1 << 31) - 16) {  // LdConvBwdA's 32-bit byte offsets
    set_error("batch %d too large for the conv %d input gradient", B, I);
    return MT_ERR_ARG;
  }
  const auto wg = conv_wgrad_jobs_sel<G, I == 0>(x, ws + L.dact[I], ws + (I % 2 ? L.wslab2 : L.wslab),
                                             grad + n->off_conv[I], B);
  if constexpr (I > 0) {
    constexpr int J = I - 1;
    using GJ = LayerG<Ar, J>;
    if constexpr (pooled<Ar, J>() && G::S == 1 && G::SAME && dconv_bwd_solo<G>()) {  // direct dX launch, then dW
      MT_TRY((conv_dgrad_unpool_solo<G, GJ>(ws + L.dact[I], P + n->off_conv[I], ws + L.pool[J],
                                           (const uint8_t *)(ws + L.parg[J]), ws + L.dact[J], B, act, al, s)));
      MT_TRY(launch_group(s, extra, wg.gemm, pending));
    } else if constexpr (stream_dx<G>()) {  // NATURE conv2: the weight-stationary streaming dX (nature_bwd.h)
      MT_TRY(launch_group(s, extra, DxStreamJob<G>{ws + L.dact[I], P + n->off_conv[I], ws + L.act[J], ws + L.dact[J], B,
                                            dx_stream_groups<G>(B), act, al},
                          wg.gemm, pending));
    } else if constexpr (pooled<Ar, J>()) {
      MT_TRY(launch_group(s, extra, conv_dgrad_unpool_job<G, GJ>(ws + L.dact[I], P + n->off_conv[I], ws + L.pool[J],
                                                           (const uint8_t *)(ws + L.parg[J]), ws + L.dact[J], B, act,
                                                           al),
                          wg.gemm, pending));
    } else {
      MT_TRY(launch_group(s, extra, conv_dgrad_job<G>(ws + L.dact[I], P + n->off_conv[I], ws + L.act[J], ws + L.dact[J], B,
                                               act, al),
                          wg.gemm, pending));
    }
    return trunk_backward<Ar, J>(n, P, obs, B, ws, L, grad, s, wg.sum, no);
  } else {
    MT_TRY(launch_group(s, extra, wg.gemm, pending));
    SlabJob last = wg.sum;
    if (no.partials && last.blocks() <= MT_NORM_PARTIALS / 2) {
      // conv1's slab sum writes the norm partials of its region, the rest of the gradient (complete
      // since the previous launches) is summed beside it: partials [0, slab blocks) + the rest
      last.sq = no.partials;
      const size_t b0 = n->off_conv[0], b1 = b0 + last.n;
      SumsqJob rest{grad, no.n, last.blocks() ? b0 : 0, last.blocks() ? b1 : 0, no.partials + last.blocks(),
                    MT_NORM_PARTIALS - last.blocks()};
      return launch_group(s, last, rest);
    }
    MT_TRY(launch_group(s, last));
    if (no.partials)  // (no room for the fused form: all partials from the complete gradient)
      return launch_group(s, SumsqJob{grad, no.n, 0, 0, no.partials, MT_NORM_PARTIALS});
    return MT_OK;
  }
}

// NIPS gray conv backward (nips_bwd.h): the per-image job, then the image-order slab sums of both
// layers (conv1's in region wslab, conv2's in wslab2) with the global-norm partials of the whole
// gradient when asked (the rest of the gradient, complete since the dense launch, beside them).
template <class Ar>
static int nips_conv_backward(const mt_net *n, const float *P, const uint8_t *obs, int B, float *ws,
                              const WsLayout &L, float *grad, hipStream_t s, const NormOut &no) {
  using J = NipsConvBwdJob;
  static_assert(LayerG<Ar, 0>::KK + 1 == 257 && LayerG<Ar, 1>::KK + 1 == 257, "slab rows");
  float *slab1 = ws + L.wslab, *slab2 = ws + L.wslab2;
  MT_TRY(launch_nips_conv_bwd(s, J{obs, ws + L.act[0], ws + L.dact[1], P + n->off_conv[1], ws + L.dact[0], slab1,
                                   slab2, B, n->cfg.activation, n->cfg.alpha_leaky}));
  SlabJob s1{slab1, B, (size_t)J::SLAB1, grad + n->off_conv[0]};
  SlabJob s2{slab2, (B + 1) / 2, (size_t)J::SLAB2, grad + n->off_conv[1]};  // (per image pair)
  if (!no.partials) return launch_group(s, s1, s2);
  s1.sq = no.partials;
  s2.sq = no.partials + s1.blocks();
  const int used = s1.blocks() + s2.blocks();
  static_assert(MT_NORM_PARTIALS >= 2 * ((257 * 16 / 4 + kSlabCols - 1) / kSlabCols + (257 * 32 / 4 + kSlabCols - 1) / kSlabCols),
                "norm partials");
  // (the alignment padding between the two regions is zero in both the gradient and the skip)
  return launch_group(s, s1, s2,
                      SumsqJob{grad, no.n, n->off_conv[0], n->off_conv[1] + s2.n, no.partials + used,
                               MT_NORM_PARTIALS - used});
}

// Per-row conv buffers of a layout moved to start at row `row0` (the dense/head buffers stay).
template <class Ar, int I = 0>
static void shift_rows(WsLayout &L, size_t row0) {
  if constexpr (I < Ar::NCONV) {
    using G = LayerG<Ar, I>;
    const size_t a = row0 * G::OH * G::OW * G::COUT;
    L.act[I] += a;
    L.dact[I] += a;
    if constexpr (pooled<Ar, I>()) {
      const size_t p = row0 * (G::OH / 2) * (G::OW / 2) * G::COUT;
      L.pool[I] += p;
      L.parg[I] += p / 4;
    }
    shift_rows<Ar, I + 1>(L, row0);
  }
}

// Where a forward of B rows leaves its activations: its own workspace, or rows [row0, row0+B)
// of a train workspace (tr): conv buffers through a shifted layout, H at row0.
struct ActRows {
  float *base;
  WsLayout L;
  size_t h_off;  // float offset of row 0's H from base
};
template <class Ar>
static ActRows act_rows(const mt_net *n, float *ws, const WsLayout &L, const TrainRows *tr) {
  if (!tr) return ActRows{ws, L, L.H};
  ActRows a{tr->ws, ws_layout<Ar>(n, tr->rows), 0};
  a.h_off = a.L.H + (size_t)tr->row0 * Ar::F;
  shift_rows<Ar>(a.L, (size_t)tr->row0);
  return a;
}

// BAYESIAN: where rows [row0, row0 + B) of an activation workspace keep the stage's values.
template <class Ar>
static DropoutFcArgs dropout_args(const mt_net *n, const float *P, int B, const ActRows &A, size_t row0) {
  DropoutFcArgs d{};
  d.B = B;
  d.act = n->cfg.activation;
  d.alpha = n->cfg.alpha_leaky;
  d.H3 = A.base + A.L.H3 + row0 * Ar::DROP_F;
  d.mask = reinterpret_cast<uint8_t *>(A.base + A.L.mask) + row0 * Ar::DROP_F;
  d.D = A.base + A.L.D + row0 * Ar::DROP_F;
  d.W4 = P + n->off_fc4;
  d.keep = n->cfg.keep_prob;
  return d;
}

// The end of every forward: the heads kernel finishes the dense layer's S slabs (bias, activation)
// into H and runs the heads. BAYESIAN: the dropout + fc4 stage (bayes.h) first takes fc3's slabs —
// state and counters from `ws` (the forward's own workspace), H3 / mask / D into the activation rows —
// and the heads kernel then finishes fc4's one slab into H = H4.
template <class Ar>
static int finish_forward(const mt_net *n, const float *P, int B, float *ws, const WsLayout &L, const ActRows &A,
                          const TrainRows *tr, int S, float *v, float *pi, float *rep, const SampleArgs *smp,
                          hipStream_t s) {
  const float *Wfc = P + n->off_fc;
  const float *slabs = ws + L.fcslab;
  const float *bias = Wfc + (size_t)Ar::FLAT * Ar::F;
  if constexpr (Ar::DROP_F > 0) {
    DropoutFcArgs d = dropout_args<Ar>(n, P, B, A, tr ? (size_t)tr->row0 : 0);
    d.slabs = slabs;
    d.S = S;
    d.fc_b = bias;
    d.state = reinterpret_cast<uint64_t *>(ws + L.dstate);
    d.Z4 = ws + L.z4;
    MT_TRY(launch_dropout_fc(d, s));
    slabs = d.Z4;
    S = 1;
    bias = d.W4 + (size_t)Ar::DROP_F * Ar::F;
  }
  HeadParams hp = head_params(n, P);
  return launch_heads(B, s, slabs, S, B, bias, n->cfg.activation, n->cfg.alpha_leaky, hp, n->cfg.softmax_temp,
                      A.base + A.h_off, v, pi, rep, smp ? *smp : SampleArgs{});
}

template <class Ar>
static int forward_impl(const mt_net *n, const float *P, const uint8_t *obs, int B, float *ws,
                        float *v, float *pi, float *rep, const SampleArgs *smp, hipStream_t s,
                        const TrainRows *tr = nullptr, const hipEvent_t *marks = nullptr,
                        const StackSrc *st = nullptr) {
  const WsLayout L = ws_layout<Ar>(n, B);
  const ActRows A = act_rows<Ar>(n, ws, L, tr);
  if (marks) MT_HIP(hipEventRecord(marks[0], s));
  const FwdExtras ex{st, reinterpret_cast<uint32_t *>(ws + L.sync)};
  MT_TRY((trunk_forward<Ar>(n, P, obs, B, A.base, A.L, s, ex)));
  const float *flat = layer_out<Ar, Ar::NCONV - 1>(A.base, A.L);
  // dense layer (networks.py:57-70), split-K partial slabs; heads kernel finishes bias + act.
  const float *Wfc = P + n->off_fc;
  MT_TRY((launch_fc<Ar>(flat, B, Wfc, ws + L.fcslab, L.fc_splits, s)));
  if (marks) MT_HIP(hipEventRecord(marks[1], s));
  return finish_forward<Ar>(n, P, B, ws, L, A, tr, L.fc_splits, v, pi, rep, smp, s);
}

// Inference forward (rollout steps, bootstrap): the NIPS trunk kernels where the arch has them
// (trunk_fused.h: conv -> act2, fc -> 9 slabs), whose slabs heads_fwd_kernel finishes; else the
// layered forward. st (NIPS only): stack the new state in the conv kernel (mt_rollout_step).
template <class Ar>
static int forward_infer_impl(const mt_net *n, const float *P, const uint8_t *obs, int B, float *ws,
                              float *v, float *pi, float *rep, const SampleArgs *smp, hipStream_t s,
                              const TrainRows *tr = nullptr, const StackSrc *st = nullptr,
                              const hipEvent_t *marks = nullptr) {
  if constexpr (Ar::FUSED_SLABS > 0) {
    constexpr int C = LayerG<Ar, 0>::CIN;
    using Fz = FusedNips<C>;
    const WsLayout L = ws_layout<Ar>(n, B);
    const ActRows A = act_rows<Ar>(n, ws, L, tr);
    const float *Wfc = P + n->off_fc;
    if (marks) MT_HIP(hipEventRecord(marks[0], s));
    MT_TRY((launch_nips_trunk<C>(obs, st, B, P + n->off_conv[0], P + n->off_conv[1], Wfc, n->cfg.activation,
                                 n->cfg.alpha_leaky, A.base + A.L.act[1], tr ? A.base + A.L.act[0] : nullptr,
                                 ws + L.fcslab, s)));
    MT_LAUNCHED();
    if (marks) MT_HIP(hipEventRecord(marks[1], s));
    return finish_forward<Ar>(n, P, B, ws, L, A, tr, Fz::FC_SPLITS, v, pi, rep, smp, s);
  } else {
    // (NATURE gray: conv1 stacks, trunk_forward refuses st for the other archs)
    return forward_impl<Ar>(n, P, obs, B, ws, v, pi, rep, smp, s, tr, marks, st);
  }
}

// Bootstrap forward without its heads (mt_rollout's last chain with MT_ROLLOUT_BOOT_SLABS): the
// trunk + the dense layer's split-K slabs left in ws (ws_layout(B).fcslab; NIPS: the fused trunk's
// FC_SPLITS slabs, else fc_splits), whose sum, bias, act and critic the update's loss kernel takes
// (mt_returns_loss_backward_boot). st: the NIPS stacking source; advance: the replayed rollout's
// sequence bases (the fused dense kernel advances them).
template <class Ar>
static int forward_boot_impl(const mt_net *n, const float *P, const uint8_t *obs, int B, float *ws, hipStream_t s,
                             const StackSrc *st, uint32_t *advance, uint32_t advance_by) {
  const WsLayout L = ws_layout<Ar>(n, B);
  const float *Wfc = P + n->off_fc;
  if constexpr (Ar::FUSED_SLABS > 0) {
    constexpr int C = LayerG<Ar, 0>::CIN;
    return launch_nips_trunk<C>(obs, st, B, P + n->off_conv[0], P + n->off_conv[1], Wfc, n->cfg.activation,
                                n->cfg.alpha_leaky, ws + L.act[1], nullptr, ws + L.fcslab, s, advance, advance_by);
  } else {
    if (advance && Ar::FC_ROWS == 0) {  // (refused before anything is enqueued)
      set_error("sequence-base advance: row-split dense layers only");
      return MT_ERR_UNSUPPORTED;
    }
    const FwdExtras ex{st, reinterpret_cast<uint32_t *>(ws + L.sync)};
    MT_TRY((trunk_forward<Ar>(n, P, obs, B, ws, L, s, ex)));
    return launch_fc<Ar>(layer_out<Ar, Ar::NCONV - 1>(ws, L), B, Wfc, ws + L.fcslab, L.fc_splits, s, advance,
                         advance_by);
  }
}

// The loss arguments of a backward, host side (the kernel takes them as separate pointers): the policy
// outputs and value of the rows, the indices drawn, the returns and advantages, and where the gradient
// and the optional per-row loss terms [B][4] go.
struct LossArgs {
  const float *pi, *rep, *v;
  const int32_t *a_idx, *r_idx;
  const float *y, *adv;
  float beta;
  float *grad, *loss_terms;
};

// Loss + head gradients (policy_v_network.py:25-74): writes dz, dH (masked by the trunk output's
// activation derivative); the head weight gradient (head_wgrad_job) that every caller groups into a
// later launch writes the three head (w, b) gradients, and its LDS stage bounds the batch here, before
// anything is enqueued. Every variable's gradient is overwritten by the backward (no accumulation), so
// grad is not cleared: its alignment padding must be zero once (include/manette_hip.h, mt_loss_backward).
template <class Ar>
static int loss_bwd_launch(const mt_net *n, const float *P, int B, float *ws, const WsLayout &L, const LossArgs &la,
                           hipStream_t s, const ReturnsSrc &rs = ReturnsSrc{}) {
  if (sizeof(float) * ((size_t)B + 4 * 64) > 160 * 1024) {  // HeadWgradJob::lds()
    set_error("batch %d exceeds the head-gradient LDS stage", B);
    return MT_ERR_ARG;
  }
  // loss scaling 5.0 and the batch mean (policy_v_network.py:70-74): scale = 5/B.
  const float scale = 5.0f / (float)B;
  HeadParams hp = head_params(n, P);
  if (!launch_allowed()) return MT_OK;
  const size_t lds = (size_t)hp.nq * 16;  // the head region (heads kernel: same bound)
  if (lds > kHeadRegionMaxBytes) {
    set_error("loss: head region of %zu bytes exceeds the LDS", lds);
    return MT_ERR_ARG;
  }
  static bool attr_set = false;
  if (!attr_set && lds > 64 * 1024) {
    MT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&loss_bwd_kernel<false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHeadRegionMaxBytes));
    MT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&loss_bwd_kernel<true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHeadRegionMaxBytes));
    attr_set = true;
  }
  // (rollout values only with the scan: mt_dropout_returns_loss_backward)
  MT_CHECK_ARG(!rs.v_roll || (rs.r && !rs.boot_slabs), "rollout values need the in-kernel scan with a finished v_boot");
  hipLaunchKernelGGL(rs.v_roll ? loss_bwd_kernel<true> : loss_bwd_kernel<false>, dim3(B), dim3(256), lds, s, hp,
                     ws + L.H, la.pi, la.rep, la.v, la.a_idx, la.r_idx, la.y, la.adv, la.beta, scale, n->cfg.softmax_temp,
                     n->cfg.activation, n->cfg.alpha_leaky, ws + L.dz, ws + L.dH, la.loss_terms, rs);
  MT_LAUNCHED();
  return MT_OK;
}

template <class Ar>
static HeadWgradJob head_wgrad_job(const mt_net *n, int B, float *ws, const WsLayout &L, float *grad) {
  return HeadWgradJob{ws + L.H, ws + L.dz, B, Ar::F, n->cfg.num_actions, n->cfg.num_reps,
                      grad + n->off_critic, grad + n->off_actor, grad + n->off_rep};
}

// Launches of backward_impl up to the one that completes every dense / head gradient: the loss
// kernel, then [dense dX + dense dW + head dW] — the data-parallel split of the update
// (mt_net_backward_bucket_launches; checked at run time by backward_impl under a launch window).
constexpr int kDenseBucketLaunches = 2;

// Backward of the non-LSTM archs as grouped launches (gemm.h, launch_group): each launch runs
// every product whose inputs the previous one completed — loss | dense dX + dense dW + head dW |
// per conv layer I (top down): conv dX + conv dW + the slab sum of layer I+1's dW | conv1's slab
// sum — 2 + NCONV launches (the max pools are fused into the conv products) instead of two or three per layer.
template <class Ar>
static int backward_impl(const mt_net *n, const float *P, const uint8_t *obs, int B, float *ws, const LossArgs &la,
                         hipStream_t s, const ReturnsSrc &rs = ReturnsSrc{}, const NormOut &no = NormOut{}) {
  const WsLayout L = ws_layout<Ar>(n, B);
  const int act = n->cfg.activation;
  const float al = n->cfg.alpha_leaky;
  float *grad = la.grad;
  MT_TRY(loss_bwd_launch<Ar>(n, P, B, ws, L, la, s, rs));
  constexpr int K = Ar::NCONV - 1;
  const float *flat = layer_out<Ar, K>(ws, L);
  const float *Wfc = P + n->off_fc;
  // dense dW, db: [flat, 1]^T . dH -> grad[(FLAT+1) x F]
  // (BAYESIAN: the dense layer's output gradient is dZ3, formed from the loss kernel's dH = dZ4 below)
  const float *dtop = ws + (Ar::DROP_F > 0 ? L.dz3 : L.dH);
  const auto dw = gemm_job<TileDenseW>(LdColMajor{flat, Ar::FLAT, Ar::FLAT}, LdColMajor{dtop, Ar::F, -1},
                                       EpStore{grad + n->off_fc, Ar::F}, Ar::FLAT + 1, Ar::F, B, 1);
  const HeadWgradJob hw = head_wgrad_job<Ar>(n, B, ws, L, grad);
  // dense dX: dH . W^T, masked by the last conv's activation (every trunk ends in an unpooled conv)
  static_assert(!pooled<Ar, K>(), "the trunk ends in an unpooled conv (networks.py:178-278)");
  const auto dx = gemm_job<TileDenseX>(LdRowMajor{dtop, Ar::F}, LdRowMajor{Wfc, Ar::F},
                                       EpMasked{ws + L.dact[K], flat, Ar::FLAT, act, al}, B, Ar::FLAT, Ar::F, 1);
  if constexpr (Ar::DROP_F > 0) {
    // fc4 and the dropout, one grouped launch ahead of the dense layer's: with H = H4 the loss kernel's
    // dH is dZ4, so gW4, gb4 = [D, 1]^T . dZ4 (the D the last stage stored), dZ3 = (dZ4 . W4^T) (.) m /
    // keep (.) act'(H3) (EpDropMasked: the stored mask bytes and H3's branch), and the head dW as ever.
    // The dense / head gradients therefore complete one launch later: this backward is not bucketed.
    constexpr int DF = Ar::DROP_F;
    const float *W4 = P + n->off_fc4;
    const auto dw4 = gemm_job<TileDenseW>(LdColMajor{ws + L.D, DF, DF}, LdColMajor{ws + L.dH, Ar::F, -1},
                                          EpStore{grad + n->off_fc4, Ar::F}, DF + 1, Ar::F, B, 1);
    const auto dx4 = gemm_job<TileDenseX>(
        LdRowMajor{ws + L.dH, Ar::F}, LdRowMajor{W4, Ar::F},
        EpDropMasked{ws + L.dz3, ws + L.H3, reinterpret_cast<const uint8_t *>(ws + L.mask), DF, act, al,
                     n->cfg.keep_prob},
        B, DF, Ar::F, 1);
    MT_TRY(launch_group(s, dx4, dw4, hw));
    MT_TRY(launch_group(s, dx, dw));
  } else {
    MT_TRY(launch_group(s, dx, dw, hw));
  }
  // the data-parallel split point: every dense / head gradient is complete after this launch
  // (mt_net_backward_bucket_launches; paac._bucketed_update all-reduces that bucket next)
  if (Ar::DROP_F == 0 && g_win_on && g_win_index != kDenseBucketLaunches) {
    set_error("backward: the dense / head gradients completed after launch %d, not %d", g_win_index,
              kDenseBucketLaunches);
    return MT_ERR_UNSUPPORTED;
  }
  if constexpr (nips_fused_bwd<Ar>())
    if (B <= kNipsFusedBwdMaxRows) return nips_conv_backward<Ar>(n, P, obs, B, ws, L, grad, s, no);
  return trunk_backward<Ar, K>(n, P, obs, B, ws, L, grad, s, SlabJob{}, no);
}

// BAYESIAN: the train step's fresh mask over the H3 rows of `w` (mt_dropout_redraw): the forward stage's
// kernel with the slab sum replaced by a load of the stored H3: fresh masks -> D -> Z4 -> heads; H3 and
// the conv activations are only read
template <class Ar>
static int dropout_redraw_impl(const mt_net *net, const float *params, int batch, float *w, const WsLayout &L, float *v,
                               float *pi, float *rep, hipStream_t s) {
  const ActRows A{w, L, L.H};
  DropoutFcArgs d = dropout_args<Ar>(net, params, batch, A, 0);
  d.state = reinterpret_cast<uint64_t *>(w + L.dstate);
  d.Z4 = w + L.z4;
  MT_TRY(launch_dropout_fc(d, s));
  HeadParams hp = head_params(net, params);
  return launch_heads(batch, s, d.Z4, 1, batch, d.W4 + (size_t)Ar::DROP_F * Ar::F, net->cfg.activation,
                      net->cfg.alpha_leaky, hp, net->cfg.softmax_temp, w + L.H, v, pi, rep, SampleArgs{});
}

}  // namespace mt

#include "lstm.h"

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
using namespace mt;

// The architectures built into the library — the only list of them. fn is a generic lambda called with
// the net's arch descriptor as a type tag (`using Ar = decltype(ar);`); its status is returned.
template <class Fn>
static int with_arch(const mt_net *net, const Fn &fn) {
  const int arch = net->cfg.arch, d = net->cfg.depth;
  if (arch == MT_ARCH_NIPS && d == 1) return fn(NipsArch<4>{});
  if (arch == MT_ARCH_NIPS && d == 3) return fn(NipsArch<12>{});
  if (arch == MT_ARCH_NATURE && d == 1) return fn(NatureArch<4>{});
  if (arch == MT_ARCH_NATURE && d == 3) return fn(NatureArch<12>{});
  if (arch == MT_ARCH_PWYX && d == 1) return fn(PwyxArch<4>{});
  if (arch == MT_ARCH_PWYX && d == 3) return fn(PwyxArch<12>{});
  if (arch == MT_ARCH_LSTM && d == 1) return fn(LstmArch<4>{});
  if (arch == MT_ARCH_LSTM && d == 3) return fn(LstmArch<12>{});
  if (arch == MT_ARCH_BAYESIAN && d == 1) return fn(BayesArch<4>{});
  if (arch == MT_ARCH_BAYESIAN && d == 3) return fn(BayesArch<12>{});
  set_error("arch %d depth %d not built", arch, d);
  return MT_ERR_UNSUPPORTED;
}

// MT_OK, or the refusal of a workspace shorter than its layout.
static int check_ws(size_t ws_bytes, const WsLayout &L) {
  if (ws_bytes < L.total * sizeof(float)) {
    set_error("workspace %zu < %zu bytes", ws_bytes, L.total * sizeof(float));
    return MT_ERR_WORKSPACE;
  }
  return MT_OK;
}
// The same for the layout of `batch` rows, which *L receives.
template <class Ar>
static int checked_layout(const mt_net *net, int batch, size_t ws_bytes, WsLayout *L = nullptr) {
  const WsLayout l = ws_layout<Ar>(net, batch);
  if (L) *L = l;
  return check_ws(ws_bytes, l);
}
// The same for a workspace and the bootstrap forward's (mt_returns_loss_backward_boot), refused together.
template <class Ar>
static int checked_layout_boot(const mt_net *net, int batch, size_t ws_bytes, WsLayout *L, int boot_batch,
                               size_t boot_ws_bytes, WsLayout *LB) {
  *L = ws_layout<Ar>(net, batch);
  *LB = ws_layout<Ar>(net, boot_batch);
  if (ws_bytes < L->total * sizeof(float) || boot_ws_bytes < LB->total * sizeof(float)) {
    set_error("workspace %zu / bootstrap workspace %zu < %zu / %zu bytes", ws_bytes, boot_ws_bytes,
              L->total * sizeof(float), LB->total * sizeof(float));
    return MT_ERR_WORKSPACE;
  }
  return MT_OK;
}

extern "C" int mt_net_create(const mt_net_config *cfg, mt_net **out) {
  MT_CHECK_ARG(cfg && out, "null argument");
  MT_CHECK_ARG(cfg->depth == 1 || cfg->depth == 3, "depth must be 1 or 3");
  MT_CHECK_ARG(cfg->num_actions >= 1 && cfg->num_actions <= 32, "num_actions out of range [1,32]");
  MT_CHECK_ARG(cfg->num_reps >= 1 && cfg->num_reps <= 31, "num_reps out of range [1,31]");
  MT_CHECK_ARG(cfg->activation == MT_ACT_RELU || cfg->activation == MT_ACT_LEAKY, "bad activation");
  MT_CHECK_ARG(cfg->softmax_temp > 0.f, "softmax_temp must be > 0");
  // (NaN fails both comparisons; the other archs ignore the field)
  MT_CHECK_ARG(cfg->arch != MT_ARCH_BAYESIAN || (cfg->keep_prob > 0.f && cfg->keep_prob <= 1.f),
               "keep_prob must be in (0, 1] for the BAYESIAN arch");
  mt_net *n = new mt_net();
  n->cfg = *cfg;
  n->C = 4 * cfg->depth;
  n->O = 1 + cfg->num_actions + cfg->num_reps;
  const int rc = with_arch(n, [&](auto ar) -> int {
    using Ar = decltype(ar);
    if constexpr (Ar::LSTM) build_layout_lstm<Ar>(n);
    else build_layout<Ar>(n);
    return MT_OK;
  });
  if (rc != MT_OK) {  // (the depth is 1 or 3: no such arch)
    delete n;
    set_error("arch %d not built into this library", cfg->arch);
    return rc;
  }
  *out = n;
  return MT_OK;
}

extern "C" void mt_net_destroy(mt_net *net) { delete net; }

#ifdef MT_PROBE
extern "C" int mt_probe_read(unsigned long long *out, size_t n) {
  MT_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(mt_probe_buf), std::min(n, sizeof(mt_probe_buf) / 8) * 8));
  return MT_OK;
}
extern "C" int mt_probe_read_chain(unsigned long long *out, size_t n) {
  MT_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(mt_probe_chain), std::min(n, sizeof(mt_probe_chain) / 8) * 8));
  return MT_OK;
}
extern "C" int mt_probe_read_chain_blocks(unsigned long long *out, size_t n) {
  MT_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(mt_probe_chainblk), std::min(n, sizeof(mt_probe_chainblk) / 8) * 8));
  return MT_OK;
}
#endif

extern "C" int mt_net_num_params(const mt_net *net, size_t *n) {
  MT_CHECK_ARG(net && n, "null argument");
  *n = net->nparams;
  return MT_OK;
}

extern "C" int mt_net_num_vars(const mt_net *net, int *n) {
  MT_CHECK_ARG(net && n, "null argument");
  *n = (int)net->vars.size();
  return MT_OK;
}

extern "C" int mt_net_var_info(const mt_net *net, int i, char *name, int name_len, int64_t *shape4,
                               int *ndim, size_t *offset, float *init_bound) {
  MT_CHECK_ARG(net, "null net");
  MT_CHECK_ARG(i >= 0 && i < (int)net->vars.size(), "var index %d out of range", i);
  const VarInfo &v = net->vars[i];
  if (name && name_len > 0) {
    std::strncpy(name, v.name.c_str(), name_len - 1);
    name[name_len - 1] = 0;
  }
  if (shape4)
    for (int k = 0; k < 4; ++k) shape4[k] = k < v.ndim ? v.shape[k] : 0;
  if (ndim) *ndim = v.ndim;
  if (offset) *offset = v.offset;
  if (init_bound) *init_bound = v.bound;
  return MT_OK;
}

extern "C" int mt_net_get_config(const mt_net *net, mt_net_config *cfg) {
  MT_CHECK_ARG(net && cfg, "null argument");
  *cfg = net->cfg;
  return MT_OK;
}

extern "C" int mt_net_feature_dim(const mt_net *net, int *f) {
  MT_CHECK_ARG(net && f, "null argument");
  *f = net->F;
  return MT_OK;
}

extern "C" int mt_net_workspace_bytes(const mt_net *net, int batch, size_t *bytes) {
  MT_CHECK_ARG(net && bytes, "null argument");
  MT_CHECK_ARG(batch >= 1, "batch must be >= 1");
  return with_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    *bytes = ws_layout<Ar>(net, batch).total * sizeof(float);
    return MT_OK;
  });
}

extern "C" int mt_net_backward_bucket_launches(const mt_net *net, int *launches) {
  MT_CHECK_ARG(net && launches, "null argument");
  return with_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    if constexpr (Ar::LSTM) {
      set_error("the LSTM backward is not bucketed");
      return MT_ERR_UNSUPPORTED;
    } else if constexpr (Ar::DROP_F > 0) {
      set_error("the BAYESIAN backward is not bucketed (its dense gradients complete one launch later)");
      return MT_ERR_UNSUPPORTED;
    } else {
      *launches = kDenseBucketLaunches;  // backward_impl: loss | dense dX + dense dW + head dW | convs
      return MT_OK;
    }
  });
}

// Byte range of a stored forward value in a workspace (diagnostics / parity; mt_net_workspace_region):
// kind 0 = conv layer `layer`'s stored output (post-activation; the pooled map of a pooled layer),
// kind 1 = a pooled layer's argmax bytes, kind 2 = the dense layer's post-activation output H,
// kind 3 = the conv output's gradient (the backward's dY of the layer's weight gradient),
// kind 4 = the stacking chains' hand-off counters (uint32 words, zero between launches; 0 bytes when
// the arch keeps none).
template <class Ar, int I = 0>
static int ws_region(const WsLayout &L, int kind, int layer, size_t rows, size_t *offset, size_t *bytes) {
  if (kind == 4) {
    *offset = L.sync * sizeof(float);
    *bytes = (L.total - L.sync) * sizeof(float);
    return MT_OK;
  }
  if (kind == 2) {
    *offset = L.H * sizeof(float);
    *bytes = rows * Ar::F * sizeof(float);
    return MT_OK;
  }
  if (kind >= 5) {  // BAYESIAN: the mask bytes, H3, the dropout state (bayes.h)
    if constexpr (Ar::DROP_F > 0) {
      *offset = (kind == 5 ? L.mask : kind == 6 ? L.H3 : L.dstate) * sizeof(float);
      *bytes = kind == 5 ? rows * Ar::DROP_F : kind == 6 ? rows * Ar::DROP_F * sizeof(float) : (2 + rows) * 8;
      return MT_OK;
    } else {
      set_error("regions 5-7 belong to the BAYESIAN arch");
      return MT_ERR_ARG;
    }
  }
  if constexpr (I < Ar::NCONV) {
    if (layer != I) return ws_region<Ar, I + 1>(L, kind, layer, rows, offset, bytes);
    using G = LayerG<Ar, I>;
    constexpr bool P = pooled<Ar, I>();
    const size_t px = P ? (size_t)(G::OH / 2) * (G::OW / 2) : (size_t)G::OH * G::OW;
    if (kind == 0) {
      *offset = (P ? L.pool[I] : L.act[I]) * sizeof(float);
      *bytes = rows * px * G::COUT * sizeof(float);
      return MT_OK;
    }
    if (kind == 1 && P) {
      *offset = L.parg[I] * sizeof(float);
      *bytes = rows * px * G::COUT;
      return MT_OK;
    }
    if (kind == 3) {  // the gradient of the conv output (full resolution; written by the backward)
      *offset = L.dact[I] * sizeof(float);
      *bytes = rows * G::OH * G::OW * G::COUT * sizeof(float);
      return MT_OK;
    }
    set_error("conv layer %d has no region of kind %d", layer, kind);
    return MT_ERR_ARG;
  }
  set_error("no conv layer %d", layer);
  return MT_ERR_ARG;
}

extern "C" int mt_net_workspace_region(const mt_net *net, int layout, int a, int b, int kind, int layer,
                                       size_t *offset, size_t *bytes) {
  MT_CHECK_ARG(net && offset && bytes, "null argument");
  MT_CHECK_ARG(a >= 1 && (layout != 1 || b >= 1) && kind >= 0 && kind <= 7, "bad sizes or kind");
  MT_CHECK_ARG(kind < 4 || layout == 0,
               "the counter region (kind 4) and the dropout regions (5-7) are in the layout-0 workspace");
  return with_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    if (layout == 0) {
      if constexpr (Ar::LSTM) {
        set_error("layout 0 is the non-LSTM workspace");
        return MT_ERR_ARG;
      } else {
        return ws_region<Ar>(ws_layout<Ar>(net, a), kind, layer, (size_t)a, offset, bytes);
      }
    } else if (layout == 1 || layout == 2) {
      if constexpr (!Ar::LSTM) {
        set_error("layouts 1 and 2 are LSTM workspaces");
        return MT_ERR_ARG;
      } else if (layout == 1) {  // the frame store of E = a envs, T = b steps
        const LstmFrameWs X = lstm_frame_layout<Ar>(net, a, b);
        return ws_region<Ar>(X.L, kind, layer, kind == 2 ? (size_t)X.W : (size_t)X.R_max, offset, bytes);
      } else {  // a windows of STEPS frames each
        return ws_region<Ar>(lstm_ws_layout<Ar>(net, a, nullptr), kind, layer,
                             kind == 2 ? (size_t)a : (size_t)a * Ar::STEPS, offset, bytes);
      }
    }
    set_error("layout %d", layout);
    return MT_ERR_ARG;
  });
}

extern "C" int mt_forward(const mt_net *net, const float *params, const uint8_t *obs, int batch,
                          void *ws, size_t ws_bytes, float *v, float *pi, float *rep,
                          mt_stream_t stream) {
  return mt::forward_sample(net, params, obs, batch, ws, ws_bytes, v, pi, rep, nullptr, false,
                            (hipStream_t)stream);
}

// Trunk half of the inference forward (diagnostics / roofline timing): everything up to the
// dense layer's partial slabs that heads_fwd_kernel finishes — the fused NIPS trunk, else the
// layered convs + split-K fc (LSTM: the 5B-frame trunk + the cell's x-product slabs).
template <class Ar>
static int trunk_infer_impl(const mt_net *n, const float *P, const uint8_t *obs, int B, float *ws, hipStream_t s,
                            const StackSrc *st = nullptr) {
  if constexpr (Ar::LSTM) {
    LstmWs X;
    const WsLayout L = lstm_ws_layout<Ar>(n, B, &X);
    const int rows = B * Ar::STEPS;
    MT_TRY((trunk_forward<Ar>(n, P, obs, rows, ws, L, s)));
    return launch_gemm<TileFc>(LdRowMajor{layer_out<Ar, Ar::NCONV - 1>(ws, L), Ar::FLAT},
                               LdColMajor{P + n->off_lstm, Ar::G4, -1}, EpSlab{ws + X.xg, rows, Ar::G4}, rows,
                               Ar::G4, Ar::FLAT, X.xg_splits, s);
  } else {
    const WsLayout L = ws_layout<Ar>(n, B);
    const float *Wfc = P + n->off_fc;
    if constexpr (Ar::FUSED_SLABS > 0) {
      constexpr int C = LayerG<Ar, 0>::CIN;
      MT_TRY((launch_nips_trunk<C>(obs, st, B, P + n->off_conv[0], P + n->off_conv[1], Wfc,
                                   n->cfg.activation, n->cfg.alpha_leaky, ws + L.act[1], nullptr, ws + L.fcslab, s)));
      MT_LAUNCHED();
      return MT_OK;
    } else {
      const FwdExtras ex{st, reinterpret_cast<uint32_t *>(ws + L.sync)};
      MT_TRY((trunk_forward<Ar>(n, P, obs, B, ws, L, s, ex)));
      return launch_fc<Ar>(layer_out<Ar, Ar::NCONV - 1>(ws, L), B, Wfc, ws + L.fcslab, L.fc_splits, s);
    }
  }
}

extern "C" int mt_forward_trunk(const mt_net *net, const float *params, const uint8_t *obs, int batch, void *ws,
                                size_t ws_bytes, mt_stream_t stream) {
  MT_CHECK_ARG(net && params && obs && ws, "null argument");
  MT_CHECK_ARG(batch >= 1, "batch must be >= 1");
  return with_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    MT_TRY(checked_layout<Ar>(net, batch, ws_bytes));
    return trunk_infer_impl<Ar>(net, params, obs, batch, (float *)ws, (hipStream_t)stream);
  });
}

extern "C" int mt_forward_trunk_stacking(const mt_net *net, const float *params, const uint8_t *prev,
                                         const uint8_t *frames, const uint32_t *ready, uint32_t tag, uint8_t *out,
                                         int batch, void *ws, size_t ws_bytes, uint32_t *status,
                                         mt_stream_t stream) {
  MT_CHECK_ARG(net && params && prev && frames && ready && out && ws, "null argument");
  MT_CHECK_ARG(batch >= 1, "batch must be >= 1");
  StackSrc st{prev, frames, nullptr, out};
  st.ready = ready;
  st.tag = tag & 0x1fffffffu;
  st.status = status;
  return with_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    MT_TRY(checked_layout<Ar>(net, batch, ws_bytes));
    if constexpr (Ar::LSTM) {
      set_error("stacking trunk: the NIPS, gray NATURE and PWYX archs (the LSTM steps: mt_lstm_step_forward)");
      return MT_ERR_UNSUPPORTED;
    } else if constexpr (Ar::DROP_F > 0) {
      set_error("stacking trunk: not built for the BAYESIAN arch (call mt_forward_infer on the stacked state)");
      return MT_ERR_UNSUPPORTED;
    } else {
      return trunk_infer_impl<Ar>(net, params, out, batch, (float *)ws, (hipStream_t)stream, &st);
    }
  });
}

extern "C" int mt_forward_rows(const mt_net *net, const float *params, const uint8_t *obs, int batch, void *ws,
                               size_t ws_bytes, void *train_ws, size_t train_ws_bytes, int train_rows, int row0,
                               float *v, float *pi, float *rep, mt_stream_t stream) {
  MT_CHECK_ARG(train_ws, "null train workspace");
  const TrainRows tr{(float *)train_ws, train_ws_bytes, train_rows, row0};
  return mt::forward_sample(net, params, obs, batch, ws, ws_bytes, v, pi, rep, nullptr, true, (hipStream_t)stream,
                            &tr);
}

extern "C" int mt_forward_infer(const mt_net *net, const float *params, const uint8_t *obs, int batch,
                                void *ws, size_t ws_bytes, float *v, float *pi, float *rep,
                                mt_stream_t stream) {
  return mt::forward_sample(net, params, obs, batch, ws, ws_bytes, v, pi, rep, nullptr, true,
                            (hipStream_t)stream);
}

int mt::forward_sample(const mt_net *net, const float *params, const uint8_t *obs, int batch,
                       void *ws, size_t ws_bytes, float *v, float *pi, float *rep, const SampleArgs *smp,
                       bool infer, hipStream_t stream, const TrainRows *tr, const StackSrc *st,
                       const hipEvent_t *marks) {
  MT_CHECK_ARG(net && params && obs && ws && v && pi && rep, "null argument");
  // (smp without counters: no draw — the replayed rollout graph's bootstrap carries only `advance`)
  MT_CHECK_ARG(!smp || !smp->counters || (smp->a_idx && smp->r_idx), "null sample buffer");
  MT_CHECK_ARG(batch >= 1, "batch must be >= 1");
  return with_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    MT_TRY(checked_layout<Ar>(net, batch, ws_bytes));
    if (tr) {
      MT_CHECK_ARG(!Ar::LSTM, "train-row forwards are not built for the LSTM arch (frame store: mt_lstm_*)");
      MT_CHECK_ARG(tr->ws && tr->rows >= 1 && tr->row0 >= 0 && tr->row0 + batch <= tr->rows,
                   "train rows [%d, %d) outside [0, %d)", tr->row0, tr->row0 + batch, tr->rows);
      const size_t need = ws_layout<Ar>(net, tr->rows).total * sizeof(float);
      if (tr->ws_bytes < need) {
        set_error("train workspace %zu < %zu bytes", tr->ws_bytes, need);
        return MT_ERR_WORKSPACE;
      }
    }
    if constexpr (Ar::LSTM) {
      return lstm_forward_impl<Ar>(net, params, obs, batch, (float *)ws, v, pi, rep, smp, stream);
    } else {
      MT_CHECK_ARG(!st || infer, "stacking forward is an inference forward");
      return infer ? forward_infer_impl<Ar>(net, params, obs, batch, (float *)ws, v, pi, rep, smp, stream, tr, st,
                                            marks)
                   : forward_impl<Ar>(net, params, obs, batch, (float *)ws, v, pi, rep, smp, stream, tr, marks);
    }
  });
}

int mt::forward_boot(const mt_net *net, const float *params, const uint8_t *obs, int batch, void *ws,
                     size_t ws_bytes, hipStream_t stream, const StackSrc *st, uint32_t *advance, uint32_t advance_by) {
  MT_CHECK_ARG(net && params && obs && ws && batch >= 1, "bad argument");
  return with_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    if constexpr (Ar::LSTM) {
      set_error("the LSTM bootstrap runs through mt_lstm_step_forward");
      return MT_ERR_UNSUPPORTED;
    } else {
      MT_TRY(checked_layout<Ar>(net, batch, ws_bytes));
      return forward_boot_impl<Ar>(net, params, obs, batch, (float *)ws, stream, st, advance, advance_by);
    }
  });
}

extern "C" int mt_loss_backward(const mt_net *net, const float *params, const uint8_t *obs,
                                int batch, void *ws, size_t ws_bytes, const float *pi,
                                const float *rep, const float *v, const int32_t *a_idx,
                                const int32_t *r_idx, const float *y, const float *adv,
                                float entropy_beta, float *grad, float *loss_terms,
                                mt_stream_t stream) {
  MT_CHECK_ARG(net && params && obs && ws && pi && rep && v && a_idx && r_idx && y && adv && grad,
               "null argument");
  MT_CHECK_ARG(batch >= 1, "batch must be >= 1");
  const LossArgs la{pi, rep, v, a_idx, r_idx, y, adv, entropy_beta, grad, loss_terms};
  return with_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    MT_TRY(checked_layout<Ar>(net, batch, ws_bytes));
    if constexpr (Ar::LSTM)
      return lstm_backward_impl<Ar>(net, params, obs, batch, (float *)ws, la, (hipStream_t)stream);
    else
      return backward_impl<Ar>(net, params, obs, batch, (float *)ws, la, (hipStream_t)stream);
  });
}

extern "C" int mt_dropout_redraw(const mt_net *net, const float *params, int batch, void *ws, size_t ws_bytes,
                                 float *v, float *pi, float *rep, mt_stream_t stream) {
  MT_CHECK_ARG(net && params && ws && v && pi && rep, "null argument");
  MT_CHECK_ARG(batch >= 1, "batch must be >= 1");
  return with_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    if constexpr (Ar::DROP_F == 0) {
      set_error("mt_dropout_redraw: the BAYESIAN arch only");
      return MT_ERR_UNSUPPORTED;
    } else {
      WsLayout L;
      MT_TRY(checked_layout<Ar>(net, batch, ws_bytes, &L));
      return dropout_redraw_impl<Ar>(net, params, batch, (float *)ws, L, v, pi, rep, (hipStream_t)stream);
    }
  });
}

// The fused-returns entry points (mt_returns_loss_backward, its _boot form, the BAYESIAN
// mt_dropout_returns_loss_backward) after their own refusals: the workspace check, the in-kernel scan's
// sources, the norm partials, the backward. What differs between them:
struct ReturnsForm {
  const float *v_boot = nullptr;  // V(s_T)[E], finished; or, _boot: the bootstrap forward's workspace,
  const void *boot_ws = nullptr;  // whose dense slabs the loss kernel finishes into vt_out[E]
  size_t boot_ws_bytes = 0;
  float *vt_out = nullptr;
  // BAYESIAN: the rollout's values (the advantage's), and the redraw that first writes la's v, pi, rep
  const float *v_roll = nullptr;
  float *v_new = nullptr, *pi_new = nullptr, *rep_new = nullptr;
};
template <class Ar>
static int returns_backward(const mt_net *net, const float *params, const uint8_t *obs, int T, int E, void *ws,
                            size_t ws_bytes, const float *rewards, const float *masks, double gamma, float *y,
                            float *adv, const LossArgs &la, const ReturnsForm &form, float *norm_partials,
                            hipStream_t s) {
  const int batch = T * E;
  WsLayout L, LB;
  ReturnsSrc rs;
  if (form.boot_ws) {
    MT_TRY(checked_layout_boot<Ar>(net, batch, ws_bytes, &L, E, form.boot_ws_bytes, &LB));
    MT_CHECK_ARG(Ar::F <= 512, "F > 512");
    rs.boot_slabs = (const float *)form.boot_ws + LB.fcslab;
    rs.boot_S = Ar::FUSED_SLABS > 0 ? Ar::FUSED_SLABS : LB.fc_splits;
    rs.fc_b = params + net->off_fc + (size_t)Ar::FLAT * Ar::F;
    rs.vt_out = form.vt_out;
  } else {
    MT_TRY(checked_layout<Ar>(net, batch, ws_bytes, &L));
    rs.VT = form.v_boot;
  }
  if constexpr (Ar::DROP_F > 0) {
    // the train step's fresh mask (v', pi', rep'; mask, D and H4 for the backward), then the loss kernel
    // scans with the ROLLOUT's values for the advantage and takes the critic from v'
    if (form.v_new)
      MT_TRY(dropout_redraw_impl<Ar>(net, params, batch, (float *)ws, L, form.v_new, form.pi_new, form.rep_new, s));
  }
  rs.r = rewards;
  rs.mask = masks;
  rs.gamma = gamma;
  rs.T = T;
  rs.E = E;
  rs.y_out = y;
  rs.adv_out = adv;
  rs.v_roll = form.v_roll;
  return backward_impl<Ar>(net, params, obs, batch, (float *)ws, la, s, rs, NormOut(norm_partials, net));
}

extern "C" int mt_dropout_returns_loss_backward(const mt_net *net, const float *params, const uint8_t *obs, int T,
                                                int E, void *ws, size_t ws_bytes, const float *values,
                                                const int32_t *a_idx, const int32_t *r_idx, const float *rewards,
                                                const float *masks, const float *v_boot, double gamma, float *v_out,
                                                float *pi_out, float *rep_out, float *y, float *adv,
                                                float entropy_beta, float *grad, float *loss_terms,
                                                float *norm_partials, mt_stream_t stream) {
  MT_CHECK_ARG(net && params && obs && ws && values && a_idx && r_idx && rewards && masks && v_boot && v_out &&
                   pi_out && rep_out && y && adv && grad,
               "null argument");
  MT_CHECK_ARG(T >= 1 && E >= 1 && T <= kMaxScan, "T=%d (<= %d) and E=%d must be >= 1", T, kMaxScan, E);
  const LossArgs la{pi_out, rep_out, v_out, a_idx, r_idx, y, adv, entropy_beta, grad, loss_terms};
  ReturnsForm form;
  form.v_boot = v_boot;
  form.v_roll = values;
  form.v_new = v_out;
  form.pi_new = pi_out;
  form.rep_new = rep_out;
  return with_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    if constexpr (Ar::DROP_F == 0) {
      set_error("mt_dropout_returns_loss_backward: the BAYESIAN arch only");
      return MT_ERR_UNSUPPORTED;
    } else {
      return returns_backward<Ar>(net, params, obs, T, E, ws, ws_bytes, rewards, masks, gamma, y, adv, la, form,
                                  norm_partials, (hipStream_t)stream);
    }
  });
}

extern "C" int mt_dropout_mask_host(uint64_t seed, uint64_t global_row, uint64_t counter, float keep_prob,
                                    uint8_t *out) {
  MT_CHECK_ARG(out, "null argument");
  MT_CHECK_ARG(keep_prob > 0.f && keep_prob <= 1.f, "keep_prob must be in (0, 1]");
  const uint64_t base = dropout_base(seed, global_row, counter);
  for (int f = 0; f < kDropF; ++f) out[f] = dropout_keep(dropout_word(base, f >> 2), f & 3, keep_prob) ? 1 : 0;
  return MT_OK;
}

extern "C" int mt_returns_loss_backward(const mt_net *net, const float *params, const uint8_t *obs, int T, int E,
                                        void *ws, size_t ws_bytes, const float *pi, const float *rep,
                                        const float *values, const int32_t *a_idx, const int32_t *r_idx,
                                        const float *rewards, const float *masks, const float *v_boot, double gamma,
                                        float *y, float *adv, float entropy_beta, float *grad, float *loss_terms,
                                        float *norm_partials, mt_stream_t stream) {
  MT_CHECK_ARG(net && params && obs && ws && pi && rep && values && a_idx && r_idx && rewards && masks && v_boot &&
                   y && adv && grad,
               "null argument");
  MT_CHECK_ARG(T >= 1 && E >= 1 && T <= kMaxScan, "T=%d (<= %d) and E=%d must be >= 1", T, kMaxScan, E);
  const LossArgs la{pi, rep, values, a_idx, r_idx, y, adv, entropy_beta, grad, loss_terms};
  ReturnsForm form;
  form.v_boot = v_boot;
  return with_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    if constexpr (Ar::LSTM) {
      set_error("mt_returns_loss_backward: the LSTM arch trains through mt_lstm_frames_backward");
      return MT_ERR_UNSUPPORTED;
    } else if constexpr (Ar::DROP_F > 0) {
      // one `values` array cannot be both the rollout's v (the advantage) and the redrawn v (the critic)
      set_error("mt_returns_loss_backward: the BAYESIAN arch trains through mt_returns, mt_dropout_redraw and "
                "mt_loss_backward");
      return MT_ERR_UNSUPPORTED;
    } else {
      return returns_backward<Ar>(net, params, obs, T, E, ws, ws_bytes, rewards, masks, gamma, y, adv, la, form,
                                  norm_partials, (hipStream_t)stream);
    }
  });
}

extern "C" int mt_returns_loss_backward_boot(const mt_net *net, const float *params, const uint8_t *obs, int T, int E,
                                             void *ws, size_t ws_bytes, const float *pi, const float *rep,
                                             const float *values, const int32_t *a_idx, const int32_t *r_idx,
                                             const float *rewards, const float *masks, const void *boot_ws,
                                             size_t boot_ws_bytes, float *v_boot, double gamma, float *y, float *adv,
                                             float entropy_beta, float *grad, float *loss_terms, float *norm_partials,
                                             mt_stream_t stream) {
  MT_CHECK_ARG(net && params && obs && ws && pi && rep && values && a_idx && r_idx && rewards && masks && boot_ws &&
                   v_boot && y && adv && grad,
               "null argument");
  MT_CHECK_ARG(T >= 1 && E >= 1 && T <= kMaxScan, "T=%d (<= %d) and E=%d must be >= 1", T, kMaxScan, E);
  const LossArgs la{pi, rep, values, a_idx, r_idx, y, adv, entropy_beta, grad, loss_terms};
  ReturnsForm form;
  form.boot_ws = boot_ws;
  form.boot_ws_bytes = boot_ws_bytes;
  form.vt_out = v_boot;
  return with_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    if constexpr (Ar::LSTM) {
      set_error("mt_returns_loss_backward_boot: the LSTM arch trains through mt_lstm_frames_backward");
      return MT_ERR_UNSUPPORTED;
    } else if constexpr (Ar::DROP_F > 0) {
      set_error("mt_returns_loss_backward_boot: the BAYESIAN arch trains through mt_returns, mt_dropout_redraw "
                "and mt_loss_backward");
      return MT_ERR_UNSUPPORTED;
    } else {
      return returns_backward<Ar>(net, params, obs, T, E, ws, ws_bytes, rewards, masks, gamma, y, adv, la, form,
                                  norm_partials, (hipStream_t)stream);
    }
  });
}

// ---- LSTM frame-store mode (lstm.h) ----------------------------------------------------------
// with_arch for the frame-store calls: the LSTM archs only.
template <class Fn>
static int with_lstm_arch(const mt_net *net, const Fn &fn) {
  return with_arch(net, [&](auto ar) -> int {
    if constexpr (decltype(ar)::LSTM) {
      return fn(ar);
    } else {
      set_error("frame-store calls need the LSTM arch");
      return MT_ERR_ARG;
    }
  });
}

extern "C" int mt_lstm_frames_workspace_bytes(const mt_net *net, int E, int T, size_t *bytes) {
  MT_CHECK_ARG(net && bytes, "null argument");
  MT_CHECK_ARG(E >= 1 && T >= 1, "E and T must be >= 1");
  return with_lstm_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    *bytes = lstm_frame_layout<Ar>(net, E, T).L.total * sizeof(float);
    return MT_OK;
  });
}

extern "C" int mt_lstm_frames_forward(const mt_net *net, const float *params, const uint8_t *fstore, int row0,
                                      int nrows, int E, int T, void *ws, size_t ws_bytes, mt_stream_t stream) {
  MT_CHECK_ARG(net && params && fstore && ws, "null argument");
  MT_CHECK_ARG(E >= 1 && T >= 1, "E and T must be >= 1");
  return with_lstm_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    MT_TRY(check_ws(ws_bytes, lstm_frame_layout<Ar>(net, E, T).L));
    return lstm_frames_fwd_impl<Ar>(net, params, fstore, row0, nrows, E, T, (float *)ws, (hipStream_t)stream);
  });
}

extern "C" int mt_lstm_windows_forward(const mt_net *net, const float *params, const int32_t *nz_t, int t, int E,
                                       int T, void *ws, size_t ws_bytes, float *v, float *pi, float *rep,
                                       mt_stream_t stream) {
  MT_CHECK_ARG(net && params && nz_t && ws && v && pi && rep, "null argument");
  MT_CHECK_ARG(E >= 1 && T >= 1, "E and T must be >= 1");
  return with_lstm_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    MT_TRY(check_ws(ws_bytes, lstm_frame_layout<Ar>(net, E, T).L));
    // (nz_t is only read: no nz_prev)
    return lstm_windows_fwd_impl<Ar>(net, params, const_cast<int32_t *>(nz_t), t, E, T, (float *)ws, v, pi, rep,
                                     (hipStream_t)stream);
  });
}

extern "C" int mt_lstm_step_forward(const mt_net *net, const float *params, const uint8_t *fstore, int t, int E,
                                    int T, int32_t *nz, const float *over, void *ws, size_t ws_bytes, float *v,
                                    float *pi, float *rep, mt_stream_t stream) {
  MT_CHECK_ARG(net && params && fstore && nz && ws && v && pi && rep, "null argument");
  MT_CHECK_ARG(E >= 1 && T >= 1, "E and T must be >= 1");
  return mt::lstm_step_forward(net, params, fstore, t, E, T, nz, over, ws, ws_bytes, v, pi, rep, nullptr,
                               (hipStream_t)stream);
}

int mt::lstm_step_forward(const mt_net *net, const float *params, const uint8_t *fstore, int t, int E, int T,
                          int32_t *nz, const float *over, void *ws, size_t ws_bytes, float *v, float *pi, float *rep,
                          const SampleArgs *smp, hipStream_t stream, const hipEvent_t *marks, const StackSrc *st,
                          uint32_t *sync) {
  MT_CHECK_ARG(!smp || (smp->counters && smp->a_idx && smp->r_idx), "null sample buffer");
  return with_lstm_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    MT_TRY(check_ws(ws_bytes, lstm_frame_layout<Ar>(net, E, T).L));
    return lstm_step_fwd_impl<Ar>(net, params, fstore, t, E, T, nz, over, (float *)ws, v, pi, rep, smp, stream,
                                  marks, st, sync);
  });
}

extern "C" int mt_lstm_frames_backward(const mt_net *net, const float *params, const uint8_t *fstore,
                                       const int32_t *nz, int E, int T, void *ws, size_t ws_bytes, const float *pi,
                                       const float *rep, const float *v, const int32_t *a_idx, const int32_t *r_idx,
                                       const float *y, const float *adv, float entropy_beta, float *grad,
                                       float *loss_terms, float *norm_partials, mt_stream_t stream) {
  MT_CHECK_ARG(net && params && fstore && nz && ws && pi && rep && v && a_idx && r_idx && y && adv && grad,
               "null argument");
  MT_CHECK_ARG(E >= 1 && T >= 1, "E and T must be >= 1");
  const LossArgs la{pi, rep, v, a_idx, r_idx, y, adv, entropy_beta, grad, loss_terms};
  return with_lstm_arch(net, [&](auto ar) -> int {
    using Ar = decltype(ar);
    MT_TRY(check_ws(ws_bytes, lstm_frame_layout<Ar>(net, E, T).L));
    return lstm_frames_bwd_impl<Ar>(net, params, fstore, nz, E, T, (float *)ws, la, (hipStream_t)stream,
                                    NormOut(norm_partials, net));
  });
}

// mt_sum_slabs for slabs that are not rows of float4s (n not a multiple of 4, or unaligned
// pointers): slab z starts at parts + z*n, off the 16-byte grid sum_slabs_body's vector columns
// assume (it strides the slabs by n/4 float4s). One thread per element, slabs added in slab order.
__global__ __launch_bounds__(256) void sum_slabs_scalar_kernel(const float *__restrict__ P, int S, size_t n,
                                                               float *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float t = 0.f;
  for (int z = 0; z < S; ++z) t += P[(size_t)z * n + i];
  out[i] = t;
}

extern "C" int mt_sum_slabs(const float *parts, int nslabs, size_t n, float *out,
                            mt_stream_t stream) {
  MT_CHECK_ARG(parts && out && nslabs >= 1, "bad argument");
  MT_CHECK_ARG(n >= 1 && n <= ((size_t)1 << 36), "n out of range");
  if ((n & 3) != 0 || ((((uintptr_t)parts) | ((uintptr_t)out)) & 15) != 0) {
    if (!launch_allowed()) return MT_OK;
    hipLaunchKernelGGL(sum_slabs_scalar_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       parts, nslabs, n, out);
    MT_LAUNCHED();
    return MT_OK;
  }
  return launch_group((hipStream_t)stream, SlabJob{parts, nslabs, n, out});
}
