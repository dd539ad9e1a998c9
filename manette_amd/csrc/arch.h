// Architectures of the policy/value network on gfx950: compile-time geometry, the parameter layout
// (mt_net) and the workspace layout (WsLayout), with the GEMM tiles the layouts are sized by.
//
// Reference: networks.py:130-278 (trunks). The LSTM arch extends these in lstm.h.
#pragma once
#include <string>
#include <vector>
#include <cmath>
#include <algorithm>
#include <tuple>

#include "gemm.h"
#include "jobs.h"
#include "trunk_fused.h"
#include "nips_bwd.h"
#include "dconv.h"
#include "nature_bwd.h"
#include "bayes.h"

namespace mt {

// ---------------------------------------------------------------------------------------------
// Architectures (compile-time geometry). C = 4*depth input channels. Layers = tuple of conv
// geometries; POOL bitmask = layers followed by a 2x2/2 VALID max pool (networks.py:108-110).
// ---------------------------------------------------------------------------------------------
template <int C>
struct NipsArch {  // networks.py:178-192
  using Layers = std::tuple<ConvGeom<C, 16, 8, 4, 84, 84, false>, ConvGeom<16, 32, 4, 2, 20, 20, false>>;
  static constexpr int NCONV = 2;
  static constexpr unsigned POOL = 0;
  static constexpr int FLAT = 9 * 9 * 32;  // 2592
  static constexpr int F = 256;
  static constexpr const char *FC = "fc3";
  static constexpr int FUSED_SLABS = FusedNips<C>::FC_SPLITS;  // inference forward: trunk_fused.h
  static constexpr int FC_ROWS = 0;                         // (the fused trunk has its own dense kernel)
  static constexpr bool LSTM = false;
  static constexpr int DROP_F = 0;
};
// networks.py:194-204: the NIPS trunk, then tf.nn.dropout(fc3) -> fc4 256 -> 256 (bayes.h) under the
// heads. NIPS geometry, so the fused inference trunk and the fused gray conv backward apply unchanged.
template <int C>
struct BayesArch : NipsArch<C> {
  static constexpr int DROP_F = kDropF;  // the extra stage: dropout over fc3's features + fc4
  static_assert(NipsArch<C>::F == kDropF, "dropout_fc_kernel is built for 256 features");
};
template <int C>
struct NatureArch {  // networks.py:261-278
  using Layers = std::tuple<ConvGeom<C, 32, 8, 4, 84, 84, false>, ConvGeom<32, 64, 4, 2, 20, 20, false>,
                            ConvGeom<64, 64, 3, 1, 9, 9, false>>;
  static constexpr int NCONV = 3;
  static constexpr unsigned POOL = 0;
  static constexpr int FLAT = 7 * 7 * 64;  // 3136
  static constexpr int F = 512;
  static constexpr const char *FC = "fc4";
  static constexpr int FUSED_SLABS = 0;  // no fused inference trunk: layered path
  static constexpr int FC_ROWS = 7;      // dense layer by conv3 rows (row_fc_kernel)
  // its K-splits (= slabs): 8, 512 blocks at E = 32 / 64 (two per CU) instead of 7 rows' 448
  // (Breakout isolated step forward 39.5 -> 38.5 us; 4 splits, 256 blocks: slower; profiles/r06fcs)
  static constexpr int FC_SPLITS = 8;
  static constexpr bool LSTM = false;
  static constexpr int DROP_F = 0;
};
template <int C>
struct PwyxArch {  // networks.py:206-225: SAME convs, 2x2 pools after conv1-3
  using Layers = std::tuple<ConvGeom<C, 32, 5, 1, 84, 84, true>, ConvGeom<32, 32, 5, 1, 42, 42, true>,
                            ConvGeom<32, 64, 4, 1, 21, 21, true>, ConvGeom<64, 64, 3, 1, 10, 10, true>>;
  static constexpr int NCONV = 4;
  static constexpr unsigned POOL = 0x7;
  static constexpr int FLAT = 10 * 10 * 64;  // 6400
  static constexpr int F = 512;
  static constexpr const char *FC = "fc5";
  static constexpr int FUSED_SLABS = 0;
  static constexpr int FC_ROWS = 10;  // dense layer by conv4 rows (row_fc_kernel)
  static constexpr int FC_SPLITS = 8;  // its K-splits: 512 blocks at E = 32 (10: 640), as NATURE's
  static constexpr bool LSTM = false;
  static constexpr int DROP_F = 0;
};

template <class Ar, int I>
using LayerG = std::tuple_element_t<I, typename Ar::Layers>;

// gray NATURE: the rollout chain stacks in conv1 and runs its convs as one dataflow launch
// (dconv.h nature_chain_kernel)
template <class Ar>
constexpr bool nature_stacking() {
  if constexpr (Ar::LSTM || Ar::NCONV != 3) return false;
  else return LayerG<Ar, 0>::CIN == 4 && !LayerG<Ar, 0>::SAME;
}

// The NIPS gray trunk's conv backward as one launch of per-image workgroups (nips_bwd.h) instead of
// the layered trunk_backward.
// Its slabs are per image (257 x 16 floats each, summed serially per column), so above this batch
// the layered trunk_backward (split-K slabs capped at kSlabFloats) takes over: at the benchmarked
// batches (N = E * T <= 1,280) the fused form's two slab regions stay <= 21 MB each.
constexpr int kNipsFusedBwdMaxRows = 1280;
template <class Ar>
constexpr bool nips_fused_bwd() {
  if constexpr (Ar::LSTM || Ar::NCONV != 2 || Ar::FUSED_SLABS == 0) return false;
  else return LayerG<Ar, 0>::CIN == 4;
}
template <class Ar, int I>
constexpr bool pooled() {
  return (Ar::POOL >> I) & 1u;
}
// the frame trunks (PWYX, LSTM; gray or RGB): the rollout step's conv1 launch pulls + stacks each
// env as it is published (dconv.h stack_conv1_kernel), conv2 .. layered
template <class Ar>
constexpr bool frame_stacking() {
  using G = LayerG<Ar, 0>;
  return G::S == 1 && G::SAME && pooled<Ar, 0>() && (G::CIN == 4 || G::CIN == 12) && G::H == 84 && G::W == 84;
}
// spatial size of layer I's output after its (optional) pool
template <class Ar, int I>
constexpr int out_hw() {
  using G = LayerG<Ar, I>;
  return pooled<Ar, I>() ? G::OH / 2 : G::OH;
}

}  // namespace mt

struct VarInfo {
  std::string name;
  int ndim;
  int64_t shape[4];
  size_t offset;
  float bound;
};

struct mt_net {
  mt_net_config cfg;
  int C;       // input channels (4*depth)
  int F;       // trunk feature width
  int O;       // 1 + A + R head outputs
  int nconv;
  int flat;
  std::vector<VarInfo> vars;
  size_t nparams;
  size_t off_conv[4];  // weights offset of each conv (biases follow)
  size_t off_fc, off_critic, off_actor, off_rep;
  size_t off_lstm = 0, off_proj = 0;  // LSTM arch: cell kernel (+bias), projection w (+b)
  size_t off_fc4 = 0;                 // BAYESIAN arch: fc4 weights (biases follow)
};

namespace mt {

static size_t align64(size_t x) { return (x + 63) & ~size_t(63); }

static void add_named_pair(mt_net *n, size_t &off, const std::string &wname, const std::string &bname,
                           std::vector<int64_t> wshape, int64_t nb, float bw, float bb, size_t *woff) {
  off = align64(off);
  VarInfo w{};
  w.name = wname;
  w.ndim = (int)wshape.size();
  size_t ws = 1;
  for (int i = 0; i < w.ndim; ++i) {
    w.shape[i] = wshape[i];
    ws *= (size_t)wshape[i];
  }
  w.offset = off;
  w.bound = bw;
  VarInfo b{};
  b.name = bname;
  b.ndim = 1;
  b.shape[0] = nb;
  b.offset = off + ws;
  b.bound = bb;
  *woff = off;
  n->vars.push_back(w);
  n->vars.push_back(b);
  off = off + ws + (size_t)nb;
}

static void add_pair(mt_net *n, size_t &off, const std::string &scope, const std::string &nm,
                     std::vector<int64_t> wshape, int64_t nb, float bw, float bb, size_t *woff) {
  add_named_pair(n, off, scope + "/" + nm + "/" + nm + "_weights", scope + "/" + nm + "/" + nm + "_biases",
                 std::move(wshape), nb, bw, bb, woff);
}

template <class G>
static void add_conv(mt_net *n, size_t &off, int idx) {
  // networks.py:34-55: weights U(+-1/sqrt(filters*k*k)) (shape[3] is the OUTPUT channel count),
  // biases U(+-1/sqrt(in_channels*k*k)).
  const float bw = (float)(1.0 / std::sqrt((double)(G::COUT * G::KH * G::KW)));
  const float bb = (float)(1.0 / std::sqrt((double)(G::CIN * G::KH * G::KW)));
  std::string nm = "conv" + std::to_string(idx + 1);
  add_pair(n, off, "Network", nm, {G::KH, G::KW, G::CIN, G::COUT}, G::COUT, bw, bb,
           &n->off_conv[idx]);
}

template <class Ar, int I = 0>
static void add_convs(mt_net *n, size_t &off) {
  if constexpr (I < Ar::NCONV) {
    add_conv<LayerG<Ar, I>>(n, off, I);
    add_convs<Ar, I + 1>(n, off);
  }
}

template <class Ar>
static void add_heads(mt_net *n, size_t &off) {
  const float bh = (float)(1.0 / std::sqrt((double)Ar::F));
  const int A = n->cfg.num_actions, R = n->cfg.num_reps;
  // policy_v_network.py:22 (critic), :31 (actor), :47 (repetition) — TF creation order.
  add_pair(n, off, "Training/Critic", "critic_output", {Ar::F, 1}, 1, bh, bh, &n->off_critic);
  add_pair(n, off, "Training/Actor", "actor_output", {Ar::F, A}, A, bh, bh, &n->off_actor);
  add_pair(n, off, "Training/Repetition", "repetition_output", {Ar::F, R}, R, bh, bh, &n->off_rep);
}

template <class Ar>
static void build_layout(mt_net *n) {
  static_assert(out_hw<Ar, Ar::NCONV - 1>() * out_hw<Ar, Ar::NCONV - 1>() *
                    LayerG<Ar, Ar::NCONV - 1>::COUT == Ar::FLAT, "flatten width");
  size_t off = 0;
  add_convs<Ar>(n, off);
  const float bf = (float)(1.0 / std::sqrt((double)Ar::FLAT));  // networks.py:72-89
  add_pair(n, off, "Network", Ar::FC, {Ar::FLAT, Ar::F}, Ar::F, bf, bf, &n->off_fc);
  if constexpr (Ar::DROP_F > 0) {
    // fc4 is built inside a second `with tf.name_scope('Network')`, which TF 1.x uniquifies to
    // Network_1 (TF's published behaviour; no BAYESIAN checkpoint pins it, as for the LSTM names)
    const float b4 = (float)(1.0 / std::sqrt((double)Ar::DROP_F));
    add_named_pair(n, off, "Network_1/fc4/fc4_weights", "Network_1/fc4/fc4_biases", {Ar::DROP_F, Ar::F}, Ar::F, b4,
                   b4, &n->off_fc4);
  }
  add_heads<Ar>(n, off);
  n->nparams = align64(off);
  n->F = Ar::F;
  n->flat = Ar::FLAT;
  n->nconv = Ar::NCONV;
}

// ---------------------------------------------------------------------------------------------
// Workspace layout (floats), a pure function of (net, batch).
// ---------------------------------------------------------------------------------------------
struct WsLayout {
  // per conv layer: act = post-activation conv output (unpooled layers), pool = pooled output and
  // parg = its window argmax bytes (pooled layers: the conv epilogue pools, EpBiasActPool), dact =
  // the gradient of the conv output (pre-activation after masking; full resolution)
  size_t act[4], pool[4], parg[4], dact[4], fcslab, H, dz, dH, wslab, wslab2, total;
  size_t sync;  // the stacking chains' counters (nature_chain_kernel, stack_conv1_kernel; u32, zero between launches)
  // BAYESIAN (bayes.h): fc3's output, the mask bytes, the dropped features D, fc4's one-slab product,
  // fc3's output gradient and the dropout state {seed, row0, counters[B]} (uint64)
  size_t H3 = 0, mask = 0, D = 0, z4 = 0, dz3 = 0, dstate = 0;
  int fc_splits;
};

template <int N, int BK>
struct TileFor {
  using T = Tile<64, 64, 2, 2, BK>;
};
// Thin-N conv tiles (COUT or CIN of 16 / 32): the 4 waves split M, one 16-row fragment each
// (128 / 256-row thin tiles measured slower). BK is capped so the A stage stays <= 96 KB.
constexpr int kThinBM = 64;
constexpr int thin_bk(int bk) { return kThinBM * (bk + 4) * 4 > 98304 && bk % 32 == 0 ? thin_bk(bk / 2) : bk; }
template <int BK>
struct TileFor<16, BK> {
  using T = Tile<kThinBM, 16, 4, 1, thin_bk(BK)>;
};
template <int BK>
struct TileFor<32, BK> {
  using T = Tile<kThinBM, 32, 4, 1, thin_bk(BK)>;
};

// K-chunk of a forward conv: the whole K when it fits 256, else the largest of 256/192/128
// dividing it (one fill per chunk, all loads of a chunk in flight together).
template <int K>
constexpr int conv_bk() {
  return K <= 256 ? ((K + 15) / 16) * 16 : (K % 256 == 0 ? 256 : (K % 192 == 0 ? 192 : 128));
}

template <class G>
using TileConvFwd = typename TileFor<G::COUT, conv_bk<G::KK>()>::T;
template <class G>
using TileConvWgrad = typename TileFor<G::COUT, 64>::T;
// dX: BK 64 = half the LDS of 128, twice the resident workgroups (LSTM conv2 dX -5 %, Pong conv2 dX -7 %);
// 32 for the 64-channel inputs (LSTM conv4 group 59.6 -> 56.1 us, NATURE conv3 39.6 -> 38.7; the thin
// CIN-32 tile is slower at 32: LSTM conv3 181.6 -> 190.8, profiles/r06dg)
template <class G>
using TileConvDgrad = typename TileFor<G::CIN, G::CIN >= 64 ? 32 : 64>::T;

using TileFc = Tile<32, 64, 2, 2, 64>;       // dense forward, M = batch (small), split-K
// dense dW (GEMM-K = batch: 160 = 2 chunks at ec=32) and dX (GEMM-K = F, M = batch): latency-bound
// at rollout batches, so small tiles — more workgroups, fewer MFMAs per wave (Pong: dense group
// 12.1 -> 10.6 us; LSTM dense dW 17.1 -> 13.1 us)
using TileDenseW = Tile<32, 64, 2, 2, 80>;
using TileDenseX = Tile<32, 32, 2, 2, 128>;

static int pick_splits(int grid_mn, int K, int bk, int target = 512) {
  int s = target / (grid_mn > 0 ? grid_mn : 1);
  if (s < 1) s = 1;
  const int chunks = cdiv(K, bk);
  if (s > chunks) s = chunks;
  return s;
}

// K splits of a conv weight gradient (GEMM-K = B*OH*OW, tiny M x N): enough that a block walks
// at most kWgradChunks BK-chunks (each chunk is one load latency: with only M x N / 1024 MFMA
// tiles per wave the chunk chain, not the MFMA, sets a block's time), capped so the partial slabs
// stay <= kSlabFloats.
// (4 K-chunks of 64 per block: re-checked against 1, 2, 8, 16 — DESIGN §8)
constexpr int kWgradChunks = 4;
constexpr size_t kSlabFloats = (size_t)4 << 20;
template <class G>
static int conv_wgrad_splits(int B) {
  using T = TileConvWgrad<G>;
  const int M = G::KK + 1;
  const int K = B * G::OH * G::OW;
  int s = std::max(pick_splits(cdiv(M, T::BM) * cdiv(G::COUT, T::BN), K, T::BK), cdiv(cdiv(K, T::BK), kWgradChunks));
  s = std::min<int>(s, (int)std::max<size_t>(kSlabFloats / ((size_t)M * G::COUT), 1));
  return gemm_splits<T>(K, s);
}

template <class G>
static size_t conv_wgrad_slab(int B) {
  const int s = conv_wgrad_splits<G>(B);
  const size_t generic = s > 1 ? (size_t)s * (G::KK + 1) * G::COUT : 0;
  if constexpr (dconv_wgrad<G>())  // direct weight gradient (dconv.h)
    return std::max(generic, dwgrad_slab_floats<G, false>(B));
  return generic;
}

template <class Ar>
static int fc_splits(int B, int F) {
  if constexpr (Ar::FC_ROWS > 0) return Ar::FC_SPLITS;  // row_fc_kernel's K-splits
  const int s = pick_splits(cdiv(B, TileFc::BM) * cdiv(F, TileFc::BN), Ar::FLAT, TileFc::BK, 128);
  return gemm_splits<TileFc>(Ar::FLAT, s);
}

// The dense layer's partial slabs [splits][B][F] of the inference forwards: the row-split kernel
// (trunk_fused.h row_fc_kernel: one slab per conv output row, one memory round trip per block)
// where the arch has FC_ROWS, else the split-K GEMM. advance: the replayed rollout graph's
// sequence bases (row_fc_kernel's block 0).
template <class Ar>
static int launch_fc(const float *flat, int B, const float *Wfc, float *slabs, int splits, hipStream_t s,
                     uint32_t *advance = nullptr, uint32_t advance_by = 0) {
  if constexpr (Ar::FC_ROWS > 0)
    return launch_row_fc<Ar::FLAT / Ar::FC_ROWS, Ar::FC_ROWS, Ar::F, Ar::FC_SPLITS>(flat, B, Wfc, slabs, s, advance,
                                                                                  advance_by);
  else
    return launch_gemm<TileFc>(LdRowMajor{flat, Ar::FLAT}, LdColMajor{Wfc, Ar::F, -1}, EpSlab{slabs, B, Ar::F}, B,
                               Ar::F, Ar::FLAT, splits, s);
}

template <class Ar, int I = 0>
static void ws_layers(WsLayout &L, size_t &off, int B, size_t &wslab) {
  if constexpr (I < Ar::NCONV) {
    using G = LayerG<Ar, I>;
    auto take = [&](size_t nf) {
      size_t o = off;
      off = align64(off + nf);
      return o;
    };
    const size_t a = (size_t)B * G::OH * G::OW * G::COUT;
    const size_t p = pooled<Ar, I>() ? (size_t)B * (G::OH / 2) * (G::OW / 2) * G::COUT : 0;
    L.act[I] = take(pooled<Ar, I>() ? 0 : a);
    L.dact[I] = take(a);
    L.pool[I] = take(p);
    L.parg[I] = take(p / 4);  // bytes (COUT % 4 == 0)
    wslab = std::max(wslab, conv_wgrad_slab<G>(B));
    ws_layers<Ar, I + 1>(L, off, B, wslab);
  }
}

struct LstmWs;
template <class Ar>
static WsLayout lstm_ws_layout(const mt_net *n, int B, LstmWs *X);  // lstm.h

template <class Ar>
static WsLayout ws_layout(const mt_net *n, int B) {
  if constexpr (Ar::LSTM) return lstm_ws_layout<Ar>(n, B, nullptr);
  WsLayout L{};
  size_t off = 0;
  auto take = [&](size_t nf) {
    size_t o = off;
    off = align64(off + nf);
    return o;
  };
  size_t wslab = 0;
  ws_layers<Ar>(L, off, B, wslab);
  if constexpr (nips_fused_bwd<Ar>())  // per-image conv1 slabs (wslab), per-pair conv2 slabs (wslab2)
    if (B <= kNipsFusedBwdMaxRows)
      wslab = std::max(wslab, std::max((size_t)B * NipsConvBwdJob::SLAB1, (size_t)((B + 1) / 2) * NipsConvBwdJob::SLAB2));
  L.fc_splits = fc_splits<Ar>(B, Ar::F);
  L.fcslab = take((size_t)std::max(L.fc_splits, Ar::FUSED_SLABS) * B * Ar::F);
  L.H = take((size_t)B * Ar::F);
  L.dz = take((size_t)B * n->O);
  L.dH = take((size_t)B * Ar::F);
  L.wslab = take(wslab);
  L.wslab2 = take(wslab);  // ping-pong slab regions of consecutive conv layers (trunk_backward)
  if constexpr (Ar::DROP_F > 0) {
    L.H3 = take((size_t)B * Ar::DROP_F);
    L.mask = take((size_t)B * Ar::DROP_F / 4);  // bytes
    L.D = take((size_t)B * Ar::DROP_F);
    L.z4 = take((size_t)B * Ar::F);
    L.dz3 = take((size_t)B * Ar::DROP_F);
    L.dstate = take(2 * (size_t)(2 + B));  // uint64 words
  }
  // the rollout chains' counters (nature_chain_kernel; stack_conv1_kernel), zero between launches
  L.sync = take(nature_stacking<Ar>() ? (size_t)kChainSyncWords * B
                                      : frame_stacking<Ar>() && !Ar::LSTM ? (size_t)stack_conv1_sync_words(B) : 0);
  L.total = off;
  return L;
}

}  // namespace mt
