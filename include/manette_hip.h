/*
 * manette_hip.h — C ABI of libmanette_hip.so, the MI355X (gfx950) device side of the
 * PAAC+FiGAR rollout/update hot path.
 *
 * Conventions (every entry point):
 *   - returns int status, MT_OK (0) on success; mt_last_error() gives the message of the
 *     last failure on the calling thread;
 *   - every buffer is a caller-owned DEVICE pointer unless the name says _host; the library
 *     never allocates or synchronises inside a launch function, so each call can be captured
 *     into a hipGraph (mt_graph_*);
 *   - `stream` is a hipStream_t (NULL = the legacy default stream);
 *   - tensors are dense, row-major, NHWC for images, TF variable layouts for parameters
 *     (conv HWIO, dense (in, out)), fp32 arithmetic.
 *
 * Which reference interface each entry point replaces is cited per function
 * (paths relative to the reference repo andres-quintela/manette).
 */
#ifndef MANETTE_HIP_H
#define MANETTE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *mt_stream_t; /* hipStream_t */

enum {
  MT_OK = 0,
  MT_ERR_ARG = 1,         /* bad argument (shape, null pointer, out of range) */
  MT_ERR_HIP = 2,         /* a HIP runtime call failed */
  MT_ERR_UNSUPPORTED = 3, /* configuration not built into this library */
  MT_ERR_WORKSPACE = 4    /* workspace smaller than mt_net_workspace_bytes() */
};

/* --arch values of train.py:100 (networks.py:178-278). */
enum { MT_ARCH_NIPS = 0, MT_ARCH_NATURE = 1, MT_ARCH_PWYX = 2, MT_ARCH_LSTM = 3, MT_ARCH_BAYESIAN = 4 };
/* --activation values of train.py:117 (networks.py:27-31). */
enum { MT_ACT_RELU = 0, MT_ACT_LEAKY = 1 };
/* --clip_norm_type values of train.py:96 (actor_learner.py:55-72). */
enum { MT_CLIP_IGNORE = 0, MT_CLIP_GLOBAL = 1 };

/* Number of fp32 partial sums mt_grad_sumsq writes (and mt_clip_rmsprop reads). */
#define MT_NORM_PARTIALS 512

/* Network configuration: the `network_conf` dict of train.py:52-63. */
typedef struct mt_net_config {
  int32_t arch;          /* MT_ARCH_* */
  int32_t depth;         /* 1 = gray, 3 = --rgb; input channels = 4*depth (networks.py:152) */
  int32_t num_actions;   /* A: ALE minimal action set size (environment_creator.py:28) */
  int32_t num_reps;      /* R = --nb_choices (exploration_policy.py:48) */
  int32_t activation;    /* MT_ACT_* */
  float alpha_leaky;     /* --alpha_leaky_relu */
  float softmax_temp;    /* --softmax_temp (networks.py:91-98) */
  float keep_prob;       /* --keep_percentage: BAYESIAN only, 0 < keep_prob <= 1 (the other archs ignore it) */
} mt_net_config;

typedef struct mt_net mt_net;

const char *mt_last_error(void);
int mt_version(void);

/* ---- network description / parameter layout -------------------------------------------
 * Replaces the TF graph construction of networks.py:130-278 + policy_v_network.py:19-57.
 * Parameters live in ONE flat fp32 buffer, variables in TF creation order (trunk, critic,
 * actor, repetition), each (weights, biases) pair contiguous, each pair 64-float aligned.
 * The gradient, RMSProp `ms` and `mom` slot buffers share that layout. */
int mt_net_create(const mt_net_config *cfg, mt_net **out);
void mt_net_destroy(mt_net *net);
int mt_net_num_params(const mt_net *net, size_t *n_floats);
int mt_net_num_vars(const mt_net *net, int *n);
/* TF variable name (e.g. "Network/conv1/conv1_weights"), shape, offset into the flat buffer,
 * and the uniform init bound d (networks.py:34-89: U(-d, d)); d < 0 means N(0,1) init. */
int mt_net_var_info(const mt_net *net, int i, char *name, int name_len, int64_t *shape4,
                    int *ndim, size_t *offset, float *init_bound);
int mt_net_feature_dim(const mt_net *net, int *f); /* width of the trunk output (256/512/...) */
int mt_net_get_config(const mt_net *net, mt_net_config *cfg);
/* Bytes of device workspace a forward/backward on `batch` rows needs. Zero-fill a workspace once
 * when it is allocated: the stacking chains keep per-env hand-off counters in it — the gray NATURE
 * chain (nature_chain_kernel) and the PWYX stacking conv1 launch, gray or RGB (stack_conv1_kernel) —
 * which every launch leaves at zero again, a launch whose bounded waits timed out included.
 * Scratch contract (tests/test_scratch_contract_gpu.py): of a workspace — this one, and the LSTM frame
 * store's (mt_lstm_frames_workspace_bytes), which has neither counters nor dropout state and needs no
 * zero-fill — only those counters (mt_net_workspace_region kind 4) and the BAYESIAN dropout state (kind
 * 7) persist between calls; of the other buffers only the once-zeroed alignment padding of `grad`
 * (mt_loss_backward). Every other workspace word is scratch: a call reads only what it, or the call the
 * header names as its predecessor on the same rows (a forward before its backward, steps 0 .. t-1 of an
 * LSTM rollout), wrote, so outputs and gradients are the same bits whatever a workspace, an output or
 * the variables' ranges of `grad` held before. All of it is fp32 except the max-pool argmax bytes (kind
 * 1), the counters, the dropout mask bytes (kind 5) and the dropout state. No call writes outside the
 * sizes reported here, or past the rows of an output it was given. */
int mt_net_workspace_bytes(const mt_net *net, int batch, size_t *bytes);
/* Diagnostics / parity: where a workspace keeps a forward value the backward branches on — kind 0:
 * conv layer `layer`'s stored output, post-activation ([rows][OH][OW][COUT] fp32; a pooled layer's
 * pooled map [rows][OH/2][OW/2][COUT]), whose sign is the ReLU branch; kind 1: a pooled layer's 2x2
 * max-pool argmax bytes ([rows][OH/2][OW/2][COUT] uint8, the window position 0..3 of the first
 * maximum in (row, col) order that the backward routes the gradient to, TF MaxPoolGrad); kind 2:
 * the dense layer's output H ([rows][F] fp32); kind 3: the gradient of conv layer `layer`'s output
 * after a backward ([rows][OH][OW][COUT] fp32, full resolution); kind 4: the stacking chains' hand-off
 * counters (uint32 words, zero between launches; empty for an arch without them); kinds 5-7 (BAYESIAN,
 * layout 0): the dropout mask bytes, H3 and the dropout state, described below. Byte offset and size. layout 0 = the workspace of
 * mt_forward / mt_forward_rows on a = batch rows; layout 1 = the LSTM frame-store workspace of
 * (E = a, T = b), conv rows = fstore rows, H rows = the (T+1)E windows; layout 2 = the LSTM
 * mt_forward workspace of a windows, conv rows = window frames (window-major, 5 per window). */
int mt_net_workspace_region(const mt_net *net, int layout, int a, int b, int kind, int layer, size_t *offset,
                            size_t *bytes);

/* ---- BAYESIAN arch (networks.py:194-204, policy_v_network.py:80-81) ------------------------
 * The NIPS trunk (conv1, conv2, fc3 2592 -> 256, activation), then
 *   D  = tf.nn.dropout(H3, keep_prob)   binary = floor(keep_prob + U[0,1)), D = (H3 / keep_prob) * binary
 *                                       (an fp32 division; keep_prob == 1: D = H3, no mask, no division)
 *   H4 = act(D @ W4 + b4)               fc4 256 -> 256, variables Network_1/fc4/fc4_{weights,biases}
 * and the three heads on H4. Dropout has no training switch in the reference: every forward draws a
 * mask, and the train step draws a fresh one (mt_dropout_redraw). These TensorFlow facts (the dropout
 * formula, the Network_1 scope name, the creation order conv1, conv2, fc3, fc4, critic, actor,
 * repetition) are TF 1.x's published behaviour, not pinned by a checkpoint — as the LSTM names.
 *
 * Mask of one row (256 features), counter-based and salted away from mt_sample's stream; mix64 is
 * splitmix64's finaliser (z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb;
 * z ^= z >> 31):
 *   base = mix64(seed ^ mix64((global_row << 40) ^ counter) ^ 0xD6E8FEB86659FD93)
 *   for q in 0..63:  h = mix64(base + (q + 1) * 0x9e3779b97f4a7c15)
 *     features 4q .. 4q+3 take h's four 16-bit fields, low field first: u = field * 2^-16 (exact in fp32)
 *     keep  iff  keep_prob + u >= 1.0f    (one fp32 add: TF's floor(keep_prob + uniform))
 *   keep_prob == 1: every feature kept.
 * The dropout state lives in the workspace (mt_net_workspace_region kind 7, layout 0):
 * {uint64 seed; uint64 row0; uint64 counters[rows]}. Row b's mask is keyed on (seed, row0 + b,
 * counters[b]) and the stage increments counters[b], so each call site (workspace) has its own stream
 * and every call draws fresh masks; the zero-filled state (seed 0) is valid. Further regions: kind 5 =
 * the mask bytes [rows][256] uint8 (0 / 1), kind 6 = H3 [rows][256] fp32 (fc3 after bias and
 * activation, before dropout); kind 2 stays the features the heads read (H4).
 * mt_forward, mt_forward_infer and mt_forward_rows run the stage (mt_forward_rows: state and counters
 * of the batch-row `ws`; H3, mask and H4 land in the train rows); mt_loss_backward runs its backward
 * under the mask the workspace holds. The update in one call is mt_dropout_returns_loss_backward
 * (redraw + n-step scan + loss + backward). mt_returns_loss_backward[_boot], mt_forward_trunk_stacking
 * and mt_net_backward_bucket_launches return MT_ERR_UNSUPPORTED.
 * The native macro-step is opt-in: mt_rollout_create returns MT_ERR_UNSUPPORTED for this arch unless
 * flags carry MT_ROLLOUT_DROPOUT. With the bit, every staging / pipelining mode of a NIPS net is
 * accepted except MT_ROLLOUT_BOOT_SLABS (MT_ERR_ARG: V(s_T) needs the stage, so the bootstrap chain runs
 * stage + heads). Each step forward t = 0..T-1 and then the bootstrap draw from the dropout state of the
 * rollout's `ws`, one counter value per row each — from the replayed rollout graph too: the stream is
 * device state, never a kernel argument — and steps t < T leave H3, mask, D and H4 in train rows t*E..,
 * as mt_forward_rows does. */

/* out[256] = the mask of (seed, global_row, counter) at keep_prob, 0 / 1 (host restatement of the
 * formula above; the kernels are pinned against it). */
int mt_dropout_mask_host(uint64_t seed, uint64_t global_row, uint64_t counter, float keep_prob, uint8_t *out);

/* The train step's fresh mask (the forward inside train_step, policy_v_network.py:25-74): from the
 * H3 a forward left in rows [0, batch) of `ws`, draw new masks -> D -> fc4 -> heads into v, pi, rep,
 * leaving the fresh mask and H4 in `ws` for the following mt_loss_backward. Neither H3 nor any conv
 * activation is written. BAYESIAN only (MT_ERR_UNSUPPORTED otherwise). */
int mt_dropout_redraw(const mt_net *net, const float *params, int batch, void *ws, size_t ws_bytes, float *v,
                      float *pi, float *rep, mt_stream_t stream);

/* The BAYESIAN update's backward in one call (batch = T*E rows t*E+e): mt_returns + mt_dropout_redraw +
 * mt_loss_backward (+ mt_grad_sumsq with norm_partials), bit for bit. Launches: the redraw stage over
 * the H3 rows a rollout left in `ws` (fresh masks, one counter value per row), the heads kernel (v_out
 * [T*E], pi_out, rep_out = v', pi', rep'), then the loss kernel, whose block of row (t, e) runs env e's
 * n-step scan itself (mt_returns' arithmetic) and takes adv = R - values[t][e] — the ROLLOUT's value —
 * while the critic term and loss_terms use v'[t][e]; then the backward's grouped launches. rewards /
 * masks [T][E] may be pinned host memory read in place. y, adv [T][E] are written. norm_partials (may be
 * NULL): as mt_returns_loss_backward's. No allocation, no synchronisation: capturable. BAYESIAN only
 * (MT_ERR_UNSUPPORTED otherwise). */
int mt_dropout_returns_loss_backward(const mt_net *net, const float *params, const uint8_t *obs, int T, int E,
                                     void *ws, size_t ws_bytes, const float *values, const int32_t *a_idx,
                                     const int32_t *r_idx, const float *rewards, const float *masks,
                                     const float *v_boot, double gamma, float *v_out, float *pi_out, float *rep_out,
                                     float *y, float *adv, float entropy_beta, float *grad, float *loss_terms,
                                     float *norm_partials, mt_stream_t stream);

/* ---- forward (A5-A7) ----------------------------------------------------------------------
 * Replaces session.run([output_layer_v, output_layer_pi, output_layer_rep], {input_ph: s})
 * (paac.py:144-146, :219-224) and the forward half of train_step (paac.py:254-256).
 * obs: [batch][84][84][4*depth] uint8 (for LSTM: [batch][5][84][84][4*depth]).
 * Outputs v [batch], pi [batch][A], rep [batch][R] (softmax probabilities).
 * Activations are kept in `ws` for a following mt_loss_backward on the same rows. */
int mt_forward(const mt_net *net, const float *params, const uint8_t *obs, int batch, void *ws,
               size_t ws_bytes, float *v, float *pi, float *rep, mt_stream_t stream);

/* ---- inference forward (rollout steps, bootstrap V(s_T)) -----------------------------------
 * Same outputs as mt_forward (paac.py:144-146, :219-224) but keeps no activations for a backward
 * pass, so the NIPS arch runs its rollout trunk (manette_amd/csrc/trunk_fused.h: one conv kernel,
 * conv1 -> conv2 per (env, conv2 row) block, then the dense layer as its own MFMA GEMM kernel
 * writing 9 split-K slabs) followed by the heads kernel; other arches take mt_forward's layered
 * path. Same workspace size as mt_forward. (A one-launch variant whose last block per env
 * finished the heads measured 25 us vs 12.7 + 6.1 us: the release/acquire fences and the serial
 * tail cost more than the second launch.) */
int mt_forward_infer(const mt_net *net, const float *params, const uint8_t *obs, int batch, void *ws,
                     size_t ws_bytes, float *v, float *pi, float *rep, mt_stream_t stream);

/* Inference forward of `batch` rows that ALSO leaves their activations (and dense outputs H) in
 * rows [row0, row0 + batch) of a train workspace sized for train_rows rows
 * (mt_net_workspace_bytes(net, train_rows)). A rollout that forwards state slot t with
 * row0 = t*E fills the whole batch the update trains on (paac.py:236: row t*E + e), with the
 * parameters unchanged in between, so mt_loss_backward(train_rows) then needs no mt_forward: pass
 * it the rollout's v / pi / rep of every row. `ws` (batch rows) holds the split-K partials.
 * Not for the LSTM arch (its frame store does the same, mt_lstm_*). */
int mt_forward_rows(const mt_net *net, const float *params, const uint8_t *obs, int batch, void *ws,
                    size_t ws_bytes, void *train_ws, size_t train_ws_bytes, int train_rows, int row0, float *v,
                    float *pi, float *rep, mt_stream_t stream);

/* Trunk half of mt_forward_infer alone (roofline timing / diagnostics): the convs and the dense
 * layer's partial products, left in `ws` (NIPS: the conv kernel + the dense kernel). */
int mt_forward_trunk(const mt_net *net, const float *params, const uint8_t *obs, int batch, void *ws,
                     size_t ws_bytes, mt_stream_t stream);

/* The rollout chain's stacking trunk alone (roofline timing, parity tests): the conv kernel in its
 * in-kernel-pull form — per env, wait until ready[e * MH_READY_STRIDE] >> 3 == tag (one 128-B line
 * per env, manette_host.h), stack out = prev shifted by the push count (its low 3 bits) + that
 * many final frames (frames = [4*batch][84][84][depth], env e's pushes at slots 4e..; host-mapped
 * pinned staging or device memory) — then the dense layer's split-K partials, left in ws. NIPS:
 * nips_conv_kernel<STACK> + nips_fc_kernel; gray NATURE: nature_chain_kernel (stacking conv1 ->
 * conv2 -> conv3, per-env hand-offs in one launch) + the split-K dense GEMM; PWYX (gray or RGB):
 * stack_conv1_kernel (per-env pull + stack blocks, then conv1 tiles per env) + conv2 .. + the dense
 * GEMM. With every ready word already set nothing waits: the kernels' own duration.
 * Every device wait is bounded (~2 s): a wait that times out stores 1 into *status (a device-visible
 * word, e.g. mapped pinned memory; may be NULL) and the launch drains (an env never published keeps
 * its previous state); the caller reads *status after the stream has completed.
 * MT_ERR_UNSUPPORTED for the other archs (the LSTM steps stack in mt_rollout_step). */
int mt_forward_trunk_stacking(const mt_net *net, const float *params, const uint8_t *prev, const uint8_t *frames,
                              const uint32_t *ready, uint32_t tag, uint8_t *out, int batch, void *ws, size_t ws_bytes,
                              uint32_t *status, mt_stream_t stream);

/* ---- LSTM frame-store mode (the learner's LSTM path; manette_amd/csrc/lstm.h) -------------
 * The reference feeds each step's memory window [E][5][84][84][C] (paac.py:79-83) and the train
 * step the T*E windows of whole_memory (paac.py:233-234); consecutive windows share 4 frames.
 * Here the caller keeps ONE frame store fstore [1 + (T+5)*E][84][84][C] uint8: row 0 = zeros,
 * row 1 + slot*E + e = env e's state in slot `slot` (slots 0..3 = the previous rollout's last 4
 * states, slot 4 + t = the state before step t), and per window only nz = its number of leading
 * zero frames (reference memory[e] = 0 at an episode end, then shifted). Window (t, e) reads
 * zero frames at positions k < nz[t][e] and slot t + k otherwise.
 *  - mt_lstm_frames_forward: trunk + the cell's x-product of frame rows [row0, row0+nrows),
 *    kept in ws (step 0: rows [0, 1+5E) — zero frame + slots 0..4; step t: slot 4+t's E rows);
 *  - mt_lstm_windows_forward: the E windows of step t (t == T: the bootstrap windows) ->
 *    v [E], pi [E][A], rep [E][R] (paac.py:144-152, :219-224), nz_t = nz[t][0..E);
 *  - mt_lstm_step_forward: one macro-step of the rollout = frames_forward of step t's new rows
 *    + windows_forward of step t, with nz[t] derived on the device for t > 0 (nz [T+1][E]:
 *    nz[t][e] = over[e] != 0 ? 5 : max(nz[t-1][e] - 1, 0), `over` = step t-1's episode-end
 *    flags, device-readable — paac.py:173-174 update_memory, :202-203 the reset); the native
 *    rollout (mt_rollout_*) runs the same forward with the draw fused into its heads kernel.
 *    Steps run in order within a rollout (t > 0 after steps 0 .. t-1 on the same ws and
 *    parameters): step 0 stores each frame's x-product sum in ws, steps t > 0 read the 4 older
 *    frames' sums from there (mt_lstm_windows_forward always sums every frame from its slabs);
 *  - mt_lstm_frames_backward: loss + gradient of the T*E windows of steps 0..T-1 (the train
 *    step of paac.py:254-256) from the rollout's activations (unchanged parameters), with pi,
 *    rep, v [T*E] the rollout outputs; back-propagates through each distinct frame once.
 *    norm_partials (optional, [MT_NORM_PARTIALS]): as mt_returns_loss_backward's — the global-norm
 *    partials of the whole gradient from the backward's last launch (no mt_grad_sumsq needed). */
int mt_lstm_frames_workspace_bytes(const mt_net *net, int E, int T, size_t *bytes);
int mt_lstm_frames_forward(const mt_net *net, const float *params, const uint8_t *fstore, int row0, int nrows,
                           int E, int T, void *ws, size_t ws_bytes, mt_stream_t stream);
int mt_lstm_windows_forward(const mt_net *net, const float *params, const int32_t *nz_t, int t, int E, int T,
                            void *ws, size_t ws_bytes, float *v, float *pi, float *rep, mt_stream_t stream);
int mt_lstm_step_forward(const mt_net *net, const float *params, const uint8_t *fstore, int t, int E, int T,
                         int32_t *nz, const float *over, void *ws, size_t ws_bytes, float *v, float *pi,
                         float *rep, mt_stream_t stream);
int mt_lstm_frames_backward(const mt_net *net, const float *params, const uint8_t *fstore, const int32_t *nz,
                            int E, int T, void *ws, size_t ws_bytes, const float *pi, const float *rep,
                            const float *v, const int32_t *a_idx, const int32_t *r_idx, const float *y,
                            const float *adv, float entropy_beta, float *grad, float *loss_terms,
                            float *norm_partials, mt_stream_t stream);

/* ---- device multinomial sampling (perf mode of A3) -----------------------------------------
 * Replaces ExplorationPolicy.multinomial_choose (exploration_policy.py:108-116) with an
 * inverse-CDF draw on (p - float32 epsneg), the last category taking the remainder — the
 * distribution numpy's multinomial(1, p - epsneg) draws from. Uniforms come from a
 * counter-based hash of (seed, row0 + row, counters[row]); row0 = the global env id of row 0
 * (a data-parallel rank's env offset, runners.py:17-18 shard), so every env draws the same
 * stream whichever rank owns it. counters (device, one uint64 per row) are incremented by the
 * call, so a captured graph draws fresh numbers on every replay.
 * Writes int32 indices a_idx [batch], r_idx [batch], and (if pair != NULL) both again into
 * pair [2][batch] so one copy moves them to the host. */
int mt_sample(const float *pi, const float *rep, int batch, int num_actions, int num_reps,
              uint64_t seed, int row0, uint64_t *counters, int32_t *a_idx, int32_t *r_idx, int32_t *pair,
              mt_stream_t stream);

/* ---- device exploration policy (the three choosers of exploration_policy.py:78-116) ----------
 * mt_sample draws multinomially; a policy selects e_greedy_choose with its annealing
 * (exploration_policy.py:73-76, :101-108) or argmax_choose (:98-99) instead, in mt_sample_policy and
 * in the draw fused into the rollout's heads kernel (mt_rollout_set_policy). A zero-filled mt_policy
 * is mt_sample's multinomial draw, bit for bit.
 *
 * Draw rule of one row (global_row = row0 + row, counter = counters[row] before the call); every mode
 * consumes one counter value per row per call:
 *   uniforms   h  = mix64(seed ^ mix64((global_row << 40) ^ counter))      (mix64: splitmix64's finaliser,
 *              h2 = mix64(h ^ 0x9e3779b97f4a7c15)                           spelled out above)
 *              ua = (h >> 11) * 2^-53,  ur = (h2 >> 11) * 2^-53            (doubles in [0, 1))
 *   epsilon    g = (double)(counter * rows_per_call), a uint64 product      (the reference's global_step:
 *              not annealed: eps = epsilon                                  it grows by the rows of a
 *              annealed:     eps = g <= annealing_steps                     choose call, and the row's
 *                                  ? epsilon - (g * epsilon / annealing_steps) : 0.0   counter = earlier calls)
 *              in double, in this operation order (a product, a quotient, a difference: nothing a
 *              compiler can contract), so host, device and numpy agree bit for bit. Epsilon needs no
 *              host word, survives graph replay, and a data-parallel shard anneals as the union would.
 *   MULTINOMIAL  inverse CDF on (p - epsneg) as mt_sample: action from ua, repetition from ur.
 *   EGREEDY    head of size n with uniform u (action: ua, repetition: ur, independently — the
 *              reference calls e_greedy_choose once per head):
 *                u < eps:   min(n - 1, (int)floor((u / eps) * n))   (u / eps is uniform on [0, 1) given
 *                           u < eps: no second hash)
 *                otherwise: the first maximum.
 *   ARGMAX     the first maximum in index order, as np.argmax: a NaN entry counts as the maximum and
 *              the first NaN wins (EGREEDY with eps = 0).
 * Whatever the inputs, an index is in [0, n). num_reps == 1: the repetition index is 0 in every mode. */
enum { MT_POLICY_MULTINOMIAL = 0, MT_POLICY_EGREEDY = 1, MT_POLICY_ARGMAX = 2 };
typedef struct {
  int32_t mode;            /* MT_POLICY_* */
  int32_t annealed;        /* EGREEDY: 0 = constant epsilon, 1 = annealed from the row's draw counter */
  double epsilon;          /* initial epsilon, in [0, 1] */
  double annealing_steps;  /* > 0 when annealed */
  int64_t rows_per_call;   /* what the reference's global_step grows by per choose call (>= 1) */
} mt_policy;

/* mt_sample under a policy (NULL = multinomial). MT_ERR_ARG, before any launch, for a mode outside
 * 0..2, an epsilon outside [0, 1] or NaN, annealing_steps <= 0 (or NaN) when annealed, or
 * rows_per_call < 1 in a mode other than MULTINOMIAL (the zero-filled policy stays valid). */
int mt_sample_policy(const mt_policy *policy, const float *pi, const float *rep, int batch, int num_actions,
                     int num_reps, uint64_t seed, int row0, uint64_t *counters, int32_t *a_idx, int32_t *r_idx,
                     int32_t *pair, mt_stream_t stream);
/* Host restatement of the rule above for one row, all three modes (pi, rep: HOST pointers); needs no
 * GPU. The kernels are pinned against it. */
int mt_policy_draw_host(const mt_policy *policy, uint64_t seed, uint64_t global_row, uint64_t counter,
                        const float *pi, int num_actions, const float *rep, int num_reps, int32_t *a, int32_t *r);

/* ---- n-step return / advantage scan (A9) ---------------------------------------------------
 * Replaces paac.py:219-231 (+ flatten :237-238). rewards/masks/values: [T][E] fp32,
 * v_boot: [E] (V(s_T)). Writes y, adv: [T][E] fp32 (row t*E+e). Arithmetic follows the
 * reference's numpy dtypes exactly (gamma is the python float: the first product gamma*V_T in
 * fp32, the rest fp64, fp32 output). */
/* rewards / masks may be device addresses of pinned host memory (the learner's [2][T][E]
 * bookkeeping output, read in place). */
int mt_returns(const float *rewards, const float *masks, const float *values, const float *v_boot,
               double gamma, int T, int E, float *y, float *adv, mt_stream_t stream);

/* ---- fused loss + backward (A10) ------------------------------------------------------------
 * Replaces optimizer.compute_gradients(network.loss) (actor_learner.py:49) with the loss of
 * policy_v_network.py:25-74. Requires the activations of mt_forward(obs, batch) in `ws`
 * (pi, rep, v as that call returned them). a_idx/r_idx: selected action / repetition index
 * (argmax of the one-hot feeds, paac.py:239-240). Overwrites every variable's gradient in the
 * flat `grad` and never touches its alignment padding, which the caller zeroes once when it
 * allocates grad (the clip's global norm sums the whole buffer). Also writes per-row loss terms
 * loss_terms [batch][4] = (critic 0.25(y-v)^2, -adv*(logpi_a+logrep_r), entropy_pi, entropy_rep). */
int mt_loss_backward(const mt_net *net, const float *params, const uint8_t *obs, int batch,
                     void *ws, size_t ws_bytes, const float *pi, const float *rep, const float *v,
                     const int32_t *a_idx, const int32_t *r_idx, const float *y, const float *adv,
                     float entropy_beta, float *grad, float *loss_terms, mt_stream_t stream);

/* mt_returns + mt_loss_backward in one call (the update of a rollout, batch = T*E rows t*E+e):
 * the loss kernel block of row (t, e) runs the n-step scan of env e from T-1 down to t itself
 * (the same arithmetic as mt_returns, bit for bit) — one launch fewer on the update's critical
 * path. y and adv ([T][E]) are still written. values: [T][E] = the v the rollout returned.
 * norm_partials (may be NULL): also write the MT_NORM_PARTIALS global-norm partials of the
 * gradient, as mt_grad_sumsq(grad, n, 1.0f) would for mt_clip_rmsprop (no data-parallel
 * all-reduce in between); the sum of squares is taken in the backward's last launch. */
int mt_returns_loss_backward(const mt_net *net, const float *params, const uint8_t *obs, int T, int E, void *ws,
                             size_t ws_bytes, const float *pi, const float *rep, const float *values,
                             const int32_t *a_idx, const int32_t *r_idx, const float *rewards,
                             const float *masks, const float *v_boot, double gamma, float *y, float *adv,
                             float entropy_beta, float *grad, float *loss_terms, float *norm_partials,
                             mt_stream_t stream);
/* mt_returns_loss_backward with the bootstrap finished here: boot_ws is the rollout's E-row
 * inference workspace whose dense-layer slabs the last chain left (MT_ROLLOUT_BOOT_SLABS); each
 * loss block sums env e's slabs in slab order, adds the bias, applies the activation and takes the
 * critic's dot product (the heads kernel's arithmetic) for V(s_T)[e] = v_boot[e] (written out),
 * then scans. Same outputs as mt_returns_loss_backward given that v_boot. */
int mt_returns_loss_backward_boot(const mt_net *net, const float *params, const uint8_t *obs, int T, int E, void *ws,
                                  size_t ws_bytes, const float *pi, const float *rep, const float *values,
                                  const int32_t *a_idx, const int32_t *r_idx, const float *rewards,
                                  const float *masks, const void *boot_ws, size_t boot_ws_bytes, float *v_boot,
                                  double gamma, float *y, float *adv, float entropy_beta, float *grad,
                                  float *loss_terms, float *norm_partials, mt_stream_t stream);

/* ---- global-norm clip + TF1 ApplyRMSProp (A11) ----------------------------------------------
 * Replaces clip_by_global_norm (actor_learner.py:59-63) + ApplyRMSProp (actor_learner.py:47-48,74).
 * mt_grad_sumsq writes MT_NORM_PARTIALS fp32 partial sums of (inv_scale*g)^2.
 * mt_clip_rmsprop: g' = inv_scale*g; norm = sqrt(sum partials);
 *   clip_type GLOBAL: g' *= clip * min(1/norm, 1/clip);
 *   ms += (g'^2 - ms)*(1 - decay); mom = momentum*mom + g'*lr/sqrt(ms + eps); w -= mom.
 * lr is read by the kernel from *lr_dev (device memory, or — as the learner does — the device
 * address of pinned host memory the host writes the schedule into, actor_learner.py:132-136), so
 * no copy is needed and a captured graph picks up the schedule. norm_out (device, may be NULL)
 * receives the pre-clip norm.
 * inv_scale folds the 1/world of a data-parallel all-reduce (sum) into the update. */
int mt_grad_sumsq(const float *g, size_t n, float inv_scale, float *partials, mt_stream_t stream);
int mt_clip_rmsprop(float *w, float *ms, float *mom, const float *g, size_t n,
                    const float *partials, const float *lr_dev, float decay, float momentum,
                    float eps, float clip, int clip_type, float inv_scale, float *norm_out,
                    mt_stream_t stream);

/* ---- frame preprocess + 4-frame stack (A2) --------------------------------------------------
 * Replaces AtariEmulator.__process_frame_pool / ObservationPool (atari_emulator.py:79-88,
 * environment.py:58-80): per env, each "push" is the pair of the last two ALE screens of one
 * emulator.next() (atari_emulator.py:90-100): pooled = max(f0, f1) (np.amax), resized to 84x84
 * with the nearest LUT (row_lut[84], col_lut[84] = source row/col), appended to the 4-deep
 * observation stack. Per env e: push_offset[e], push_count[e] (1..4) index the pushes (oldest
 * first) in `raw` = [total_pushes][2][src_rows][160][depth] uint8: whole screens (src_rows 210,
 * row_lut = the resize LUT) or the 84 rows the resize reads, staged by the runner (src_rows 84,
 * row_lut = identity). prev/out: [E][84][84][4*depth];
 * out[c] = prev[c+p] for c < 4-p, else the (c-(4-p))-th new push; RGB interleaves channels as
 * [R_t0..R_t3, G_t0..G_t3, B_t0..B_t3] (environment.py:75). out may not alias prev. */
int mt_preprocess(const uint8_t *raw, const int32_t *push_offset, const int32_t *push_count,
                  int E, int depth, int src_rows, const int32_t *row_lut, const int32_t *col_lut,
                  const uint8_t *prev, uint8_t *out, mt_stream_t stream);

/* Pooled variant: each staging slot holds ONE screen per push, max(f0, f1) already taken on the
 * host by the emulator's frame pool (mh_runner MH_RUNNER_POOLED): raw = [slots][src_rows][160][depth]. */
int mt_preprocess_pooled(const uint8_t *raw, const int32_t *push_offset, const int32_t *push_count,
                         int E, int depth, int src_rows, const int32_t *row_lut, const int32_t *col_lut,
                         const uint8_t *prev, uint8_t *out, mt_stream_t stream);

/* Resized variant (MT_ROLLOUT_RESIZED): staging slot push_offset[e] + j holds push j's FINAL
 * 84x84xdepth frame, pooled and resized by the host threads (mh_runner MH_RUNNER_RESIZED):
 * frames = [slots][84][84][depth]; the kernel only stacks it onto prev. */
int mt_preprocess_resized(const uint8_t *frames, const int32_t *push_offset, const int32_t *push_count, int E,
                          int depth, const uint8_t *prev, uint8_t *out, mt_stream_t stream);

/* In-place variant (MT_ROLLOUT_IN_PLACE): the pushes' screens are read where the emulators left
 * them. screens = a bank of whole 210-row screens [..][210][160][depth] (pinned + device-mapped
 * host memory, or device memory); push j's frame f of env e is screen frame_idx[e*8 + 2j + f]
 * (j < push_count[e]), as mh_runner_step_frames writes them (include/manette_host.h). Only the
 * 84 rows row_lut names are read. */
int mt_preprocess_frames(const uint8_t *screens, const int32_t *frame_idx, const int32_t *push_count,
                         int E, int depth, const int32_t *row_lut, const int32_t *col_lut,
                         const uint8_t *prev, uint8_t *out, mt_stream_t stream);

/* Device address of pinned (page-locked, mapped) host memory, e.g. an emulator screen bank. */
int mt_host_device_pointer(void *host, void **dev);

/* ---- LSTM memory window (paac.py:79-83 update_memory + :202-203 episode-end reset) --------
 * memory [E][5][frame] (the window each env's forward reads), whole_t [E][5][frame] = row t of
 * whole_memory, fresh [E][frame] = the new states, masks [E] = 1 - episode_over (float32).
 * whole_t <- memory; memory <- shift left + fresh; memory[e] <- 0 where masks[e] == 0.
 * frame = 84*84*4*depth bytes. */
int mt_memory_push(uint8_t *memory, uint8_t *whole_t, const uint8_t *fresh, const float *masks, int E,
                   size_t frame_bytes, mt_stream_t stream);

/* ---- native rollout macro-step (orchestrates A1-A3, A8; paac.py:140-205) -------------------
 * One call = one macro-step t of every env: mt_forward on state slot t with the A3 draw fused
 * into its heads kernel (indices into idx[0][t], idx[1][t] and the [2][E] pair) -> wait for the
 * pair (spin on the stream's event) -> mh_runner_step (native emulator threads,
 * libmanette_host.so) -> mh_book_step (bookkeeping into rm_host[.][t]) -> mt_preprocess of the
 * pushed screens into state slot t+1.
 * flags = 0: the pair is copied D2H and the screens + push metadata H2D (hipMemcpyAsync).
 * flags & MT_ROLLOUT_IN_PLACE (implies ZERO_COPY): no screen is staged at all — the emulators run
 * mh_runner_step_frames and mt_preprocess_frames reads their screens in place: staging_host is
 * then the emulators' screen bank (pinned, device-mapped), frames_host [E][8] the frame indices
 * and meta_host[E..2E) the push counts.
 * flags & MT_ROLLOUT_ZERO_COPY: the heads kernel writes the pair into pair_host and the
 * preprocess kernel reads staging_host / meta_host in place (host-mapped pinned memory): no
 * copy engine and no cross-engine wait on the per-step critical path; raw / meta / pair may then
 * be null. All buffers are caller-owned; `runner` / `book` are mh_runner* / mh_book* handles. */
#define MT_ROLLOUT_ZERO_COPY 1
#define MT_ROLLOUT_IN_PLACE 2
/* flags & MT_ROLLOUT_POOLED: the runner stages ONE pooled screen per push (MH_RUNNER_POOLED) and the
 * preprocess is mt_preprocess_pooled. */
#define MT_ROLLOUT_POOLED 4
/* flags & MT_ROLLOUT_PIPELINED (needs ZERO_COPY or IN_PLACE): each call enqueues step t+1's chain
 * (a bounded device wait on sync_host[0], preprocess, forward + draw) before it waits for step t's
 * indices, and after the emulators only stores the step word — no launch on the critical path.
 * sync_host = [2] uint32 pinned + mapped: [0] host step word, [1] device wait timeout status.
 * PIPELINED + RESIZED + the NIPS arch ("stacking" rollout): the chain of step t+1 is the conv
 * kernel — each (env, row) block waits for the word the emulator thread stores once its env is
 * staged (mh_runner_set_ready), reads that env's frames from the pinned staging and stacks state
 * slot t+1 from slot t itself (no pull or preprocess launch) — the dense kernel and the heads
 * kernel, which writes each env's (a, r) as one tagged 8-byte word into host memory (no fence).
 * Every chain of a rollout is armed at its step 0 (from the second rollout on as one replayed
 * hipGraph whose sequence tags live in device memory), and step 0's forward takes slot 0 from
 * slot T of the previous rollout (the update then needs no copy). Other pipelined modes: a pull
 * kernel per env copies the frames into HBM, then the preprocess kernel, then the forward. */
#define MT_ROLLOUT_PIPELINED 8
/* flags & MT_ROLLOUT_RESIZED: the runner stages each push's final 84x84 frame (MH_RUNNER_RESIZED,
 * staging [4E][84*84*depth]) and the preprocess is mt_preprocess_resized (row/col LUTs unused). */
#define MT_ROLLOUT_RESIZED 16
/* flags & MT_ROLLOUT_BOOT_SLABS (pipelined, v_boot set, not LSTM): the last chain's bootstrap
 * forward stops after the dense layer — its split-K slabs stay in ws — and the update's loss kernel
 * finishes V(s_T) itself (mt_returns_loss_backward_boot, which writes v_boot): one heads kernel and
 * one kernel boundary fewer between the last emulator step and the backward. */
#define MT_ROLLOUT_BOOT_SLABS 32
/* flags & MT_ROLLOUT_DROPOUT: accept a BAYESIAN net (see "BAYESIAN arch" above; without the bit it is
 * refused with MT_ERR_UNSUPPORTED). MT_ERR_ARG on any other arch, and together with BOOT_SLABS. */
#define MT_ROLLOUT_DROPOUT 64
typedef struct mt_rollout mt_rollout;
typedef struct mt_rollout_buffers {
  /* device */
  uint8_t *states;             /* [T+1][E][84][84][4*depth] */
  float *values;               /* [T][E] */
  int32_t *idx;                /* [2][T][E]: action indices, then repetition indices */
  float *pi, *rep;             /* [E][A], [E][R] */
  void *ws;                    /* forward workspace for E rows */
  size_t ws_bytes;
  uint64_t *counters;          /* [E] sampling counters */
  uint8_t *raw;                /* [4E][2][src_rows*160*depth] screen staging */
  int32_t src_rows;            /* staged screen rows: 210, or 84 when the runner selects rows */
  int32_t *pair;               /* [2][E] device scratch: this step's indices for one D2H copy */
  int32_t *pair_host;          /* [2][E] pinned */
  int32_t *meta;               /* [2][E] push offsets; push counts */
  const int32_t *row_lut, *col_lut;
  /* pinned host */
  int32_t *idx_host;           /* [2][T][E] */
  uint8_t *staging_host;       /* [4E][2][src_rows*160*depth] */
  int32_t *meta_host;          /* [2][E] */
  float *reward_host, *over_host; /* [E] */
  float *rm_host;              /* [2][T][E]: clipped rewards; masks */
  int32_t *frames_host;        /* [E][8] in-place frame indices (MT_ROLLOUT_IN_PLACE), else NULL */
  uint32_t *sync_host;         /* [2] pipelined step word + wait status (MT_ROLLOUT_PIPELINED), else NULL */
  void *train_ws;              /* optional: train workspace of T*E rows; the forward of step t then also
                                  writes rows [t*E, (t+1)*E) (mt_forward_rows) and pi / rep are
                                  [T][E][.] per-step outputs; NULL: pi / rep are [E][.] */
  size_t train_ws_bytes;
  float *v_boot;               /* optional [E] (MT_ROLLOUT_PIPELINED): the last step's chain also runs the
                                  bootstrap forward of slot T (paac.py:219-224) into it, in the shadow
                                  of the host's last emulator step */
  uint32_t *ready_host;        /* [E] zero-copy modes: the heads kernel stores a step sequence number per
                                  env after writing its pair; the host polls these instead of an event
                                  (NULL: hipEventQuery) */
  int32_t flags;               /* MT_ROLLOUT_* */
  int32_t env_offset;          /* global env id of env 0 (data-parallel shard offset): the draw's row0 */
  int32_t *nz;                 /* LSTM arch only (else NULL): [T+1][E] device window zero counts; nz[0]
                                  is the caller's, step t > 0 derives nz[t] (mt_lstm_step_forward).
                                  With the LSTM arch `states` is slot 4 of a frame store
                                  [1 + (T+5)E][84][84][C] (mt_lstm_*), ws is its workspace
                                  (mt_lstm_frames_workspace_bytes), train_ws is NULL and pi / rep are
                                  [T+1][E][.] per-step outputs (row T: the bootstrap's) */
} mt_rollout_buffers;
int mt_rollout_create(const mt_net *net, int E, int T, void *runner, void *book,
                      const mt_rollout_buffers *buffers, uint64_t seed, mt_rollout **out);
void mt_rollout_destroy(mt_rollout *ro);
int mt_rollout_step(mt_rollout *ro, const float *params, int t, int64_t *global_step,
                    mt_stream_t stream);
/* The whole rollout: mt_rollout_step for t = 0 .. T-1 in one call (paac.py:140-205 without a
 * return to the caller between macro-steps). */
int mt_rollout_run(mt_rollout *ro, const float *params, int64_t *global_step, mt_stream_t stream);
/* The exploration policy of the draw fused into every step's heads kernel (mt_policy above; NULL =
 * multinomial, the default), every arch the rollout serves, LSTM included. Checked as mt_sample_policy
 * checks it. Accepted only before the rollout's first mt_rollout_step — MT_ERR_ARG after it: the
 * replayed rollout graph bakes the kernel arguments in. */
int mt_rollout_set_policy(mt_rollout *ro, const mt_policy *policy);
/* Host wall-clock microseconds accumulated by mt_rollout_step, per phase: [0] launch + wait
 * for the sampled indices, [1] emulator step, [2] bookkeeping, [3] upload + preprocess
 * enqueue, [4] number of steps. reset != 0 zeroes the counters. */
int mt_rollout_stats(mt_rollout *ro, double *out5, int reset);
/* mt_rollout_stats plus the split of [0]: out[5] = host enqueue (the step's forward and the armed
 * chains' launches), out[6] = wait for the sampled indices; n = how many of the 7 values to copy. */
int mt_rollout_stats_ex(mt_rollout *ro, double *out, int n, int reset);
/* Host timeline of the last min(max_steps, 256) macro-steps, oldest first, 6 doubles each:
 * t, then host wall microseconds at the call's start, after its launches, when the sampled
 * indices were seen, after the emulator step, after the bookkeeping (diagnostics). */
int mt_rollout_host_trace(mt_rollout *ro, double *out, int max_steps, int *n);
/* Live timing of the trunk kernels the rollout runs (roofline measurement, bench.py): enable != 0
 * records an event pair around each step forward's trunk launches (NIPS: the stacking conv kernel
 * + the dense kernel); a call with enable == 0 waits for them and returns their summed duration
 * in microseconds and their count, then stops. Any call returns (and forgets) what was recorded. */
int mt_rollout_trunk_timing(mt_rollout *ro, int enable, double *sum_us, int64_t *count);

/* Update launched by the rollout itself (native pipelined step, replayed update graph): once
 * registered, the last macro-step of every rollout (after its bookkeeping) stores
 * lr = get_lr(global_step) — actor_learner.py:145-148: initial_lr - global_step * initial_lr /
 * annealing_steps while global_step <= annealing_steps, else 0, in double, then rounded to float —
 * into *lr_host (the pinned LR word the RMSProp kernel reads) and launches graph_exec (the update:
 * loss backward [, all-reduce], clip + RMSProp) on the rollout's stream, right behind the bootstrap
 * chain: the update then starts with no host round trip after the last emulator step (the caller
 * must not launch it again). graph_exec NULL unregisters every registered update, this form's and a
 * data-parallel one (mt_rollout_set_update_dp), before the graphs are destroyed. */
int mt_rollout_set_update(mt_rollout *ro, void *graph_exec, float *lr_host, double initial_lr,
                          double annealing_steps);
/* Diagnostics: the update the rollout launches — *form = 0 none, 1 mt_rollout_set_update's graph,
 * 2 mt_rollout_set_update_dp's three graphs. */
int mt_rollout_update_form(const mt_rollout *ro, int *form);

/* ---- data-parallel communicator (RCCL over xGMI; manette_amd/csrc/comm.hip) ----------------
 * The reference has no collective: its only shard unit is the contiguous env split of
 * runners.py:17-18 (np.split over workers). This build splits envs over ranks the same way (rank r
 * owns global envs [r*ec, (r+1)*ec)) and exchanges exactly one thing per update: the flat fp32
 * gradient, summed in place (mt_allreduce) between mt_returns_loss_backward and mt_clip_rmsprop
 * (inv_scale = 1/world), i.e. the union batch's mean gradient of actor_learner.py:49 before the
 * global-norm clip of :59-63. mt_broadcast copies rank 0's parameters / RMSProp slots at start
 * (and on resume). Both are stream-ordered and capturable into a hipGraph.
 * Bootstrap: rank 0 calls mt_comm_unique_id, ships the MT_COMM_UID_BYTES bytes to every rank over
 * any control channel (the learner uses torch.distributed's gloo store), then every rank calls
 * mt_comm_init(uid, rank, world, device) collectively. */
#define MT_COMM_UID_BYTES 128
typedef struct mt_comm mt_comm;
int mt_comm_unique_id(char *uid /* [MT_COMM_UID_BYTES] */);
int mt_comm_init(const char *uid, int rank, int world, int device, mt_comm **out);
void mt_comm_destroy(mt_comm *comm);
int mt_comm_info(const mt_comm *comm, int *rank, int *world);
/* In-place sum over ranks of n fp32 values (ncclAllReduce, ncclSum). */
int mt_allreduce(mt_comm *comm, float *buf, size_t n, mt_stream_t stream);
/* In-place broadcast of `bytes` bytes from rank `root`. */
int mt_broadcast(mt_comm *comm, void *buf, size_t bytes, int root, mt_stream_t stream);
/* Diagnostics / tests: a communicator without RCCL standing for `replicas` identical ranks. Its
 * mt_allreduce multiplies the buffer by `replicas` at once (the in-place sum of identical replicas)
 * and then holds the stream for delay_us microseconds; mt_broadcast is a no-op. A sum that started
 * before its producer finished, or a consumer that did not wait for it, changes the result (the
 * stream-order tests of the data-parallel update, tests/test_dp_gpu.py). */
int mt_comm_init_loopback(int replicas, int delay_us, mt_comm **out);

/* The data-parallel update launched by the rollout itself (the counterpart of mt_rollout_set_update
 * for world > 1, or forced at world 1): once registered, the last macro-step of every rollout stores
 * the LR as mt_rollout_set_update does and enqueues, with no return to the caller,
 *   graph_execs[0] (loss + dense / head gradients: the backward's first
 *   mt_net_backward_bucket_launches launches) on the rollout's stream;
 *   the in-place sum of grad[split, n) (mt_allreduce) on a side stream the rollout owns, behind it;
 *   graph_execs[1] (the rest of the conv backward) on the rollout's stream;
 *   the sum of grad[0, split) on the side stream, behind that;
 *   graph_execs[2] (norm partials + clip + RMSProp with inv_scale = 1/world) behind both sums.
 * The all-reduces run beside the conv backward, as PAACLearner._bucketed_update issues them from
 * Python (which the learner keeps for communicators outside the C ABI). graph_execs NULL
 * unregisters; registering either form replaces the other. */
int mt_rollout_set_update_dp(mt_rollout *ro, void *const *graph_execs, mt_comm *comm, float *grad, size_t n,
                             size_t split, float *lr_host, double initial_lr, double annealing_steps);

/* ---- small helpers ----------------------------------------------------------------------- */
/* out[i] = sum_z parts[z*n + i] (deterministic order); used for split reductions. The order, for
 * n a multiple of 4 and 16-byte aligned parts / out: the 16 subset sums s_k = sum of the slabs
 * z = k, k + 16, ... (in slab order) added as s_0 + s_1 + ... + s_15, which is plain slab order
 * up to 16 slabs; otherwise (slabs off the 16-byte grid) plain slab order, one element per thread. */
int mt_sum_slabs(const float *parts, int nslabs, size_t n, float *out, mt_stream_t stream);

/* Launch window: after mt_launch_window(first, count), first >= 0, the library numbers its grouped
 * launches, loss-kernel launches and every launch of mt_lstm_frames_backward from 0 in issue order and issues only those with index in
 * [first, first + count) (count < 0: no upper end); the others return MT_OK without launching.
 * mt_launch_window(-1, -1), the default, turns it off. Used while CAPTURING: one
 * mt_returns_loss_backward* call recorded as two graphs, [0, 2) = the loss + the dense / head
 * gradient launch and [2, ...) = the conv backward, so a data-parallel learner all-reduces the
 * dense / head bucket while the conv backward runs (paac.py); and by bench.py to time a backward
 * launch by launch. Library-global: set it around calls of one thread only. Returns how many
 * launches were numbered since the previous call. */
int mt_launch_window(int first, int count);
/* How many leading launches of mt_returns_loss_backward* (non-LSTM) complete the gradient of every
 * variable from the dense layer on (the tail of the flat gradient, ~98 % of its bytes): a
 * data-parallel learner captures launches [0, n) and [n, ...) as two graphs and all-reduces the
 * tail between them while the rest of the conv backward runs. */
int mt_net_backward_bucket_launches(const mt_net *net, int *launches);

/* hipGraph capture of everything launched on `stream` between begin and end. */
int mt_graph_begin(mt_stream_t stream);
int mt_graph_end(mt_stream_t stream, void **graph_exec);
int mt_graph_launch(void *graph_exec, mt_stream_t stream);
int mt_graph_destroy(void *graph_exec);

/* ---- Catch: a device-resident environment (step, render and stack in one kernel) ------------
 * A small real game whose state lives in HBM: a paddle, falling balls, lives, three actions. The
 * counterpart of the reference's Catcher-v0 entry (pretrained/catcher/args.json), with rules of its
 * own, integer arithmetic only, so the kernel, the host restatement (mt_catch_*_host) and a numpy
 * restatement agree bit for bit. The rule:
 *
 *   field      84 x 84, background 0, x to the right, y down. The paddle is 12 wide and 3 high, rows
 *              79..81, its left edge paddle_x in [0, 72]. The ball is 4 x 4, its top-left corner
 *              (ball_x, ball_y), ball_x in [0, 80]. gray: ball 255, paddle 160; RGB: ball
 *              (255, 64, 64), paddle (64, 255, 64). Where both cover a pixel the ball is drawn.
 *   actions    0 = noop, 1 = left, 2 = right (num_actions = 3).
 *   sub-frame  1. paddle_x += (action == 1 ? -2 : action == 2 ? +2 : 0), clamped to [0, 72];
 *              2. ball_y += 2; ball_x += ball_dx; ball_x < 0: ball_x = -ball_x, ball_dx = -ball_dx;
 *                 ball_x > 80: ball_x = 160 - ball_x, ball_dx = -ball_dx;
 *              3. if ball_y + 3 >= 79 (the ball's bottom row has reached the paddle's top row): caught
 *                 iff ball_x < paddle_x + 12 and ball_x + 4 > paddle_x: reward += 1; otherwise
 *                 reward -= 1 and misses += 1. balls += 1. The episode is over iff misses >= lives or
 *                 balls >= max_balls; otherwise a new ball spawns.
 *   next(a)    4 sub-frames under action a; once the episode is over the remaining sub-frames of
 *              that next are not played. A ball needs 38 sub-frames from its spawn to the paddle, so
 *              the reward of a next is -1, 0 or +1. The observation FRAME of a next is the per-channel
 *              maximum of the renders of the positions after sub-frames 3 and 4 (the frame-pool rule of
 *              atari_emulator.py:79-100 at 84 x 84).
 *   spawn      h = mix64(seed ^ mix64((global_env << 40) ^ ball_counter) ^ 0xCA7C4BA11D0FF1E5)
 *              (mix64 and the nesting as in the sampler's uniforms, under a salt of its own);
 *              ball_x = (h & 0xffffffff) % 81, ball_dx = ((h >> 32) % 3) - 1, ball_y = 0;
 *              ball_counter += 1. ball_counter is per env and is not reset by a new game; global env
 *              ids make a data-parallel shard draw what the union would draw.
 *   new game   paddle_x = 36, misses = balls = 0, a spawn; then four next(0) whose rewards are dropped
 *              (none can occur: 16 sub-frames) and whose four frames are the initial stacked state,
 *              oldest first (get_initial_state of the reference's emulators).
 *   macro-step (emulator_runner.py:24-41) next(a) is run tab_rep[r] + 1 times, the rewards summed,
 *              stopping at the first episode end; after an episode end a new game starts at once and
 *              the state returned is its initial state (all four stack positions replaced).
 *   stacking   out[c] = prev[c + p] for c < 4 - p, else the (c - (4 - p))-th of the last p = min(pushes,
 *              4) frames, as mt_preprocess; an episode end restarts the list of pushes with the new
 *              game's four. RGB channel order [R_t0..R_t3, G_t0..G_t3, B_t0..B_t3]. */
typedef struct mt_catch_config {
  int32_t lives;     /* default 3 */
  int32_t max_balls; /* default 20 */
} mt_catch_config;
/* Per-env state, 32 bytes, in caller-owned memory. */
typedef struct mt_catch_state {
  int32_t paddle_x, ball_x, ball_y, ball_dx, misses, balls;
  uint64_t ball_counter;
} mt_catch_state;

/* A new game (ball_counter = 0 first) for envs env0 .. env0 + E - 1: state [E], out_state0
 * [E][84][84][4*depth] = the stacked initial observation. MT_ERR_ARG before any launch for E < 1,
 * env0 < 0, depth not 1 or 3, lives or max_balls < 1, or a null pointer. */
int mt_catch_reset(const mt_catch_config *cfg, uint64_t seed, int env0, int E, int depth, mt_catch_state *state,
                   uint8_t *out_state0, mt_stream_t stream);
/* One macro-step of every env, one kernel: the game logic, the renders of the pushed frames and the
 * next stacked state out [E][84][84][4*depth] from prev (no aliasing; prev is not read where all four
 * positions are replaced). tab_rep: [R] int32 (device; an entry is used clamped to [0, 255]); a_idx,
 * r_idx: [E] int32 (device), as the draw wrote them, used clamped to [0, 2] and [0, R - 1]. Writes
 * reward_out [E] (the unclipped sum) and over_out [E] (1 or 0) as fp32, and into rm_out, a [2][T][E]
 * fp32 buffer, rm_out[0][t][e] = the reward clipped to [-1, 1] and rm_out[1][t][e] = 1 - over (what
 * mt_returns* read). frames_out / push_count_out (both or neither; may be NULL): the last p = min(pushes,
 * 4) frames of env e at slots 4e .. 4e + p - 1 of frames_out [4E][84][84][depth], and p, in
 * mt_preprocess_resized's layout (push_offset[e] = 4e). MT_ERR_ARG before any launch for bad sizes
 * (E < 1, env0 < 0, R < 1, T < 1, t outside [0, T)), depth not 1 or 3, lives or max_balls < 1, out ==
 * prev, or a null required pointer. */
int mt_catch_step(const mt_catch_config *cfg, uint64_t seed, int env0, int E, int depth, const int32_t *tab_rep,
                  int R, const int32_t *a_idx, const int32_t *r_idx, mt_catch_state *state, const uint8_t *prev,
                  uint8_t *out, uint8_t *frames_out, int32_t *push_count_out, float *reward_out, float *over_out,
                  float *rm_out, int t, int T, mt_stream_t stream);
/* The same rule for ONE env on HOST pointers; needs no GPU. The kernels are pinned against these.
 * out_state0 / out (and then prev) / frames_out [4][84][84][depth] / push_count_out may be NULL:
 * nothing is rendered for a NULL pointer (statistics runs). a and r are clamped as in the kernel. */
int mt_catch_reset_host(const mt_catch_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                        mt_catch_state *state, uint8_t *out_state0);
int mt_catch_step_host(const mt_catch_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                       const int32_t *tab_rep, int R, int a, int r, mt_catch_state *state, const uint8_t *prev,
                       uint8_t *out, uint8_t *frames_out, int32_t *push_count_out, float *reward_out,
                       float *over_out);

/* ---- Bricks: a second device-resident environment (four actions, a brick wall) ----------------
 * A Breakout-like game beside Catch, through the same interface: the state in HBM, one kernel per
 * macro-step that steps, renders and stacks. (`-g breakout` stays the synthetic Atari stand-in.) Integer
 * arithmetic only, so the kernel, the host restatement (mt_bricks_*_host) and a numpy restatement agree
 * bit for bit. The rule:
 *
 *   field      84 x 84, background 0, x to the right, y down.
 *   wall       6 rows x 14 columns of bricks, each 6 wide and 3 high, filling rows 16..33 and all 84
 *              columns: brick (row r, column c) covers pixels x in [6c, 6c + 6), y in [16 + 3r, 19 + 3r) and
 *              is bit k = 14 r + c of an 84-bit bitmap, stored as bricks_lo (bits 0..63) and bricks_hi
 *              (bits 64..83; its bits 20..31 stay 0).
 *   paddle     16 wide, 3 high, rows 79..81, its left edge paddle_x in [0, 68].
 *   ball       2 x 2, its top-left corner (ball_x, ball_y), ball_x in [0, 82].
 *   colours    gray: brick row r = 90 + 20 r, paddle 160, ball 255. RGB: ball (255, 64, 64), paddle
 *              (64, 255, 64), brick rows 0..5 (200,72,72), (198,108,58), (180,122,48), (162,162,42),
 *              (72,160,72), (66,72,200). One RENDER draws the paddle, the bricks over it, the ball over both
 *              (a pixel takes the colour of the topmost sprite that covers it). Channel order is Catch's.
 *   actions    0 = noop, 1 = fire, 2 = right, 3 = left (num_actions = 4, ALE Breakout's minimal set).
 *   parked     ball_dy == 0 means the ball is parked on the paddle: the state then holds ball_dx = 0,
 *              ball_x = paddle_x + 7 and ball_y = 77 (it is drawn there and follows the paddle).
 *   serve      decided at the start of a next(a), if the ball is parked: if a == 1 or wait >= serve_wait:
 *              h = mix64(seed ^ mix64((global_env << 40) ^ serve_counter) ^ 0xB41C5B0117A11E75);
 *              serve_counter += 1; ball_x = paddle_x + 7, ball_y = 36, ball_dy = +2,
 *              ball_dx = (-2, -1, +1, +2)[(h >> 32) & 3] (wait is left as it is); otherwise wait += 1.
 *              serve_counter is per env and is not reset by a new game (as Catch's ball_counter).
 *   sub-frame  1. paddle_x += (a == 2 ? +3 : a == 3 ? -3 : 0), clamped to [0, 68];
 *              2. if the ball is parked: ball_x = paddle_x + 7 and the sub-frame ends here;
 *              3. ball_x += ball_dx; ball_x < 0: ball_x = -ball_x, ball_dx = -ball_dx;
 *                 ball_x > 82: ball_x = 164 - ball_x, ball_dx = -ball_dx;
 *              4. ball_y += ball_dy; ball_y < 0: ball_y = -ball_y, ball_dy = -ball_dy;
 *              5. brick test at the ball's leading corner cy = ball_y + (ball_dy > 0), cx = ball_x +
 *                 (ball_dx > 0): if 16 <= cy < 34 and bit 14 ((cy - 16) / 3) + cx / 6 is set: clear it,
 *                 reward += 1, ball_dy = -ball_dy; if the bitmap is now empty all 84 bits are set again;
 *              6. paddle test, if ball_dy > 0 and ball_y + 1 >= 79, with off = ball_x + 1 - paddle_x:
 *                 0 <= off <= 16: ball_dy = -2, ball_y = 77, ball_dx = (-2, -1, +1, +2)[min(3, 4 off / 17)];
 *                 otherwise lives -= 1; at lives == 0 the episode is over (the ball stays where it is);
 *                 with lives left the ball parks (ball_dy = ball_dx = 0, ball_x = paddle_x + 7, ball_y = 77)
 *                 and wait = 0.
 *   next(a)    the serve decision, then 4 sub-frames under action a (once the episode is over the
 *              remaining sub-frames of that next are not played), then nexts += 1; the episode is also over
 *              when nexts >= max_nexts. The reward of a next is 0..4. The observation FRAME of a next is the
 *              per-channel maximum of the two renders of the state (positions AND bitmap) after sub-frames
 *              3 and 4, so a brick broken in sub-frame 4 is still visible in that frame.
 *   new game   paddle_x = 34, lives = cfg.lives, nexts = wait = 0, a full wall, the ball parked. Nothing is
 *              played: the initial stacked state is four copies of that position's render.
 *   macro-step, stacking: Catch's, with a clamped to [0, 3]: next(a) is run tab_rep[r] + 1 times, the
 *              rewards summed, stopping at the first episode end, after which a new game starts at once and
 *              the state returned is its initial state (all four stack positions replaced). */
typedef struct mt_bricks_config {
  int32_t lives;      /* default 3 */
  int32_t max_nexts;  /* default 500 */
  int32_t serve_wait; /* default 4 */
} mt_bricks_config;
/* Per-env state, 56 bytes, 8-byte aligned, in caller-owned memory; the field order is part of the ABI. */
typedef struct mt_bricks_state {
  int32_t paddle_x, ball_x, ball_y, ball_dx, ball_dy, lives, nexts, wait;
  uint64_t bricks_lo;
  uint32_t bricks_hi;
  uint32_t reserved; /* written as 0 */
  uint64_t serve_counter;
} mt_bricks_state;

/* The entry points are Catch's with this game's config and state: the same argument lists, layouts
 * (rm_out [2][T][E]; frames_out / push_count_out in mt_preprocess_resized's layout), NULL rules and
 * clamping (a_idx to [0, 3]). MT_ERR_ARG before any launch for bad sizes (E < 1, env0 < 0, R < 1, T < 1,
 * t outside [0, T)), depth not 1 or 3, lives or max_nexts < 1, serve_wait < 0, out == prev, out / prev /
 * frames_out not 16-byte or state not 8-byte aligned, frames_out without push_count_out or the reverse,
 * or a null required pointer. Capturable: no allocation, no synchronisation, no atomics. */
int mt_bricks_reset(const mt_bricks_config *cfg, uint64_t seed, int env0, int E, int depth, mt_bricks_state *state,
                    uint8_t *out_state0, mt_stream_t stream);
int mt_bricks_step(const mt_bricks_config *cfg, uint64_t seed, int env0, int E, int depth, const int32_t *tab_rep,
                   int R, const int32_t *a_idx, const int32_t *r_idx, mt_bricks_state *state, const uint8_t *prev,
                   uint8_t *out, uint8_t *frames_out, int32_t *push_count_out, float *reward_out, float *over_out,
                   float *rm_out, int t, int T, mt_stream_t stream);
/* The same rule for ONE env on HOST pointers; needs no GPU (NULL frame pointers: nothing is rendered). */
int mt_bricks_reset_host(const mt_bricks_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                         mt_bricks_state *state, uint8_t *out_state0);
int mt_bricks_step_host(const mt_bricks_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                        const int32_t *tab_rep, int R, int a, int r, mt_bricks_state *state, const uint8_t *prev,
                        uint8_t *out, uint8_t *frames_out, int32_t *push_count_out, float *reward_out,
                        float *over_out);

/* ---- Tetris: the reference's own game as a third device-resident environment (five actions) ----
 * The rule of the reference's tetris.py (88-119, 147-170, 213-335) as tetris_emulator.py drives it, quirks
 * included, through Bricks' interface. Integer arithmetic only; the kernel, the host restatement
 * (mt_tetris_*_host) and a Python restatement agree field for field, and the host restatement is pinned,
 * act by act, to recordings of the reference's own code (tests/golden/tetris_rule.npz). The rule:
 *
 *   board      10 columns x 22 rows, x to the right, y down; a cell holds a colour id 0..7 (0 = empty).
 *              Row y is the word board[y], cell x its bits 3x .. 3x+2 (bits 30, 31 stay 0). Below row 21
 *              lies a floor: every cell of a row >= 22 counts as occupied, as does a column >= 10.
 *   shapes     ids 1..7, as matrices of cells (rows top-down), in tetris_shapes' order:
 *              1 = 111/010, 2 = 022/220, 3 = 330/033, 4 = 400/444, 5 = 005/555, 6 = 6666, 7 = 77/77.
 *              The falling piece is (piece, rot, x, y): shape `piece` rotated rot = 0..3 times, its matrix's
 *              top-left cell at column x, row y. One rotation of an H x W matrix gives the W x H matrix
 *              new[i][j] = old[j][W-1-i]; four give the first again (rot counts modulo 4). A piece COLLIDES
 *              at (x, y) iff one of its non-zero cells lies on an occupied cell.
 *   actions    0 = noop, 1 = left, 2 = right, 3 = manual drop, 4 = rotate (num_actions = 5).
 *              left / right: nx = x -+ 1 clamped to [0, 10 - W]; x = nx unless the piece collides at (nx, y).
 *              manual drop: reward += 1 (on every call, whether or not it locks), then DROP.
 *              rotate: rot += 1 unless the rotated piece collides at (x, y) (which covers leaving the board
 *              on the right or at the bottom).
 *   DROP       y += 1. If the piece now collides: LOCK: its non-zero cells are written into the board at
 *              (x, y - 1); the next piece spawns: piece = next_piece, rot = 0, x = (3, 3, 4) for W =
 *              (3, 4, 2) (int(5 - W/2)), y = 0, next_piece = 1 + DRAW; the game is OVER iff the spawned piece
 *              collides (tested before any row is removed, and it stays over); then every full row (no
 *              empty cell) is removed, the rows above it moving down and empty rows entering at the top;
 *              with n the number of removed rows (n <= 4; the index is clamped): lines += n, reward +=
 *              (0, 40, 100, 300, 1200)[n] x level; then, if lines >= 6 level: level += 1 (once per lock)
 *              and speed = max(1, speed - 1).
 *   act(a)     the action; then, if speed_counter % speed == 0 and the game is not over, one DROP without
 *              the point (gravity: also when the action has just locked a piece and spawned the next);
 *              then speed_counter += 1.
 *   next(a)    act(a); nexts += 1; the episode is over iff the game is over or nexts >= max_nexts (the cap
 *              is this project's: an episode that keeps clearing rows is otherwise unbounded). The reward
 *              of a next is its score difference. The observation FRAME of a next is ONE render of the
 *              state after the act (the reference draws before the action and takes the maximum of two
 *              such screens: not reproduced).
 *   DRAW       mix64(seed ^ mix64((global_env << 40) ^ piece_counter) ^ 0x7E7215B10C5D20F7) % 7, then
 *              piece_counter += 1. piece_counter is per env and is not reset by a new game (as Catch's
 *              ball_counter), so a data-parallel shard draws what the union would draw.
 *   reset      piece_counter = 0, next_piece = 1 + DRAW, then a new game.
 *   new game   an empty board, the piece spawns from next_piece as above (so a game's first piece is the
 *              previous game's next_piece), level = 1, lines = 0, speed = cfg.speed, speed_counter = 0. Then
 *              (tetris_emulator.py:63-70, 97-105) w = mix64(seed ^ mix64((global_env << 40) ^ piece_counter)
 *              ^ 0x57A27F0A17C0FFEE) % (max_start_wait + 1) times act(0) (piece_counter as it then stands, not
 *              advanced by this draw), then four act(0) whose frames are the initial stacked state, oldest
 *              first; rewards of these acts are dropped; then nexts = 0. (With max_start_wait <= 30 these
 *              at most 34 acts cannot end the game: they lock at most two pieces on an empty board.)
 *   macro-step, stacking: Catch's, with a clamped to [0, 4]: next(a) is run tab_rep[r] + 1 times (the
 *              entry clamped to [0, 255]), the rewards summed, stopping at the first episode end, after which
 *              a new game starts at once and the state returned is its initial state (all four stack
 *              positions replaced). A macro-step plays at most tab_rep[r] + 1 + 34 acts.
 *   render     84 x 84 from the reference's 288 x 396 screen (16 x 22 cells of 18 px) under a nearest
 *              resize: output pixel (row i, column j) shows cell (cx, cy) = ((((2j+1) 12) / 7) / 18,
 *              (((2i+1) 33) / 14) / 18). The colour id of a cell, later rules winning: 0; 8 where cx < 10
 *              and cx % 2 == cy % 2 (the background grid); the board's cell where it is not 0; `piece` where
 *              the falling piece has a non-zero cell; next_piece where the unrotated next piece, its
 *              matrix's top-left at cell (11, 2), has one. No text; the separator line at source x = 181 is
 *              hit by no sampled column. RGB of ids 0..8 (the reference's `colors`): (0,0,0), (255,85,85),
 *              (100,200,115), (120,108,245), (255,140,50), (50,120,52), (146,202,73), (150,161,218),
 *              (35,35,35). gray of ids 0..8: 0, 136, 160, 127, 164, 91, 171, 190, 35. Channel order is Catch's.
 *
 * A state from outside the rule is used with piece and next_piece clamped to [1, 7], rot to [0, 3], x to
 * [0, 9], y to [0, 21], level to [1, 2^20], speed to >= 1, lines to [0, 2^28], speed_counter and nexts to
 * [0, 2^30], and the board words masked to 30 bits. */
typedef struct mt_tetris_config {
  int32_t max_nexts;      /* default 2000 */
  int32_t speed;          /* default 5 (the reference's) */
  int32_t max_start_wait; /* default 0; 30 is the reference's random_start; at most 30 */
} mt_tetris_config;
/* Per-env state, 136 bytes, 8-byte aligned, in caller-owned memory; the field order is part of the ABI. */
typedef struct mt_tetris_state {
  uint32_t board[22];
  int32_t piece, rot, x, y, next_piece, level, lines, speed, speed_counter, nexts;
  uint64_t piece_counter;
} mt_tetris_state;

/* The entry points are Bricks' with this game's config and state: the same argument lists, layouts, NULL
 * rules and clamping (a_idx to [0, 4]). MT_ERR_ARG before any launch for bad sizes (E < 1, env0 < 0, R < 1,
 * T < 1, t outside [0, T)), depth not 1 or 3, max_nexts or speed < 1, max_start_wait outside [0, 30], out ==
 * prev, out / prev / frames_out not 16-byte or state not 8-byte aligned, frames_out without push_count_out
 * or the reverse, or a null required pointer. Capturable: no allocation, no synchronisation, no atomics. */
int mt_tetris_reset(const mt_tetris_config *cfg, uint64_t seed, int env0, int E, int depth, mt_tetris_state *state,
                    uint8_t *out_state0, mt_stream_t stream);
int mt_tetris_step(const mt_tetris_config *cfg, uint64_t seed, int env0, int E, int depth, const int32_t *tab_rep,
                   int R, const int32_t *a_idx, const int32_t *r_idx, mt_tetris_state *state, const uint8_t *prev,
                   uint8_t *out, uint8_t *frames_out, int32_t *push_count_out, float *reward_out, float *over_out,
                   float *rm_out, int t, int T, mt_stream_t stream);
/* The same rule for ONE env on HOST pointers; needs no GPU (NULL frame pointers: nothing is rendered). */
int mt_tetris_reset_host(const mt_tetris_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                         mt_tetris_state *state, uint8_t *out_state0);
int mt_tetris_step_host(const mt_tetris_config *cfg, uint64_t seed, uint64_t global_env, int depth,
                        const int32_t *tab_rep, int R, int a, int r, mt_tetris_state *state, const uint8_t *prev,
                        uint8_t *out, uint8_t *frames_out, int32_t *push_count_out, float *reward_out,
                        float *over_out);

/* ---- Device bookkeeping of one rollout (the learner's Bookkeeper.step, paac.py:154-205, as a kernel) ----
 * Everything a rollout of a device-resident game leaves for the host (global_step, the episode records,
 * the action / repetition histogram, the learning rate of its update) computed where the rollout ran, so
 * a training iteration needs no host synchronisation. The rule, for t = 0 .. T-1 in order, with
 * a = a_idx[t][e] clamped to [0, A-1] and r = r_idx[t][e] clamped to [0, R-1] (as the env kernel clamps):
 *
 *   per env e  total_episode_rewards[e] += reward[t][e] (one fp32 add);
 *              emulator_steps[e] += tab_rep[r] + 1 (the planned repeats, tab_rep as given);
 *              where over[t][e] != 0: append the record {global_step + env_offset + e + 1,
 *              emulator_steps[e], total_episode_rewards[e]} and zero both accumulators.
 *   order      the records of one step are appended in env order, steps in t order, record k of the
 *              book's life at ring slot k % capacity (k = words->written, which counts them).
 *   then       global_step += envs_total.
 *   after T-1  hist[a][r] = the number of (t, e) pairs that drew (a, r) and nb_actions = the sum of r + 1
 *              over the pairs: of THIS rollout (written, not accumulated); and, for g = (double)global_step,
 *              *lr = (float)(g <= lr_annealing_steps ? initial_lr - (g * initial_lr / lr_annealing_steps)
 *              : 0.0): a product, a quotient, a difference in double, rounded once to float
 *              (actor_learner.py:get_lr as the native rollout restates it).
 *   overflow   if the rollout's records would make written - acked exceed capacity, NONE of them is
 *              appended (the accumulators still advance and reset as the rule says), words->overflow is
 *              set to 1 and stays set; global_step, hist, nb_actions and *lr are written as ever.
 *              Nothing is overwritten. The host acknowledges records by storing acked = written.
 *
 * One workgroup; no atomics, no float reductions; allocates nothing, does not synchronise, capturable.
 * Every pointer is device memory (mt_book_rollout) or host memory (mt_book_rollout_host, the same rule
 * with no GPU; the kernel is pinned against it). a_idx, r_idx: [T][E] int32; reward, over: [T][E] fp32
 * (the unclipped sums and 0/1 flags of the env kernel); tab_rep: [R] int32. MT_ERR_ARG before any launch
 * for a null pointer, A, R, E or T < 1, capacity < 1, env_offset < 0, envs_total < env_offset + E, or
 * lr_annealing_steps <= 0. */
typedef struct mt_book_words {
  int64_t global_step;
  int64_t written;    /* episode records appended so far (monotonic) */
  int64_t acked;      /* stored by the host at a drain */
  int64_t nb_actions; /* of the last rollout */
  int32_t overflow;
  int32_t reserved;
} mt_book_words;
typedef struct mt_book_episode {
  int64_t global_step;
  int64_t length;
  float reward;
  int32_t reserved;
} mt_book_episode;
typedef struct mt_book_state {
  float *total_episode_rewards; /* [E] */
  int64_t *emulator_steps;      /* [E] */
  mt_book_words *words;
  int64_t *hist;                /* [A][R] */
  float *lr;                    /* the word mt_clip_rmsprop reads through lr_dev */
  mt_book_episode *ring;        /* [capacity] */
  int64_t capacity;
} mt_book_state;
int mt_book_rollout(const mt_book_state *book, const int32_t *a_idx, const int32_t *r_idx, const float *reward,
                    const float *over, const int32_t *tab_rep, int A, int R, int E, int T, int64_t env_offset,
                    int64_t envs_total, double initial_lr, double lr_annealing_steps, mt_stream_t stream);
int mt_book_rollout_host(const mt_book_state *book, const int32_t *a_idx, const int32_t *r_idx, const float *reward,
                         const float *over, const int32_t *tab_rep, int A, int R, int E, int T, int64_t env_offset,
                         int64_t envs_total, double initial_lr, double lr_annealing_steps);

/* ---- Device evaluation (K episodes on each of N envs of a device-resident game) ----------------------
 * The env kernels restart a game the moment it ends, so a fixed amount of play ("K episodes on every
 * env") needs somebody to keep the per-episode results and to stop counting an env after its K-th
 * episode. These three kernels do, in device memory: the host enqueues macro-steps (forward, draw, env
 * kernel, mt_eval_step) and reads the word block once per block of steps. The rules:
 *
 *   reset      ret_acc, len_acc, done, returns and lengths are zeroed; remaining = N * K; steps = 0.
 *   step       once after each env kernel, on that kernel's reward_out (the unclipped sum) and over_out.
 *              For env e with done[e] < K:
 *                1. ret_acc[e] += reward[e] (one fp32 add);
 *                2. len_acc[e] += clamp(tab_rep[clamp(r_idx[e], 0, R - 1)], 0, 255) + 1: the planned nexts
 *                   that Bookkeeper counts, under the env kernels' clamps;
 *                3. where over[e] != 0: returns[e][done[e]] = ret_acc[e], lengths[e][done[e]] = len_acc[e],
 *                   done[e] += 1, both accumulators zeroed.
 *              An env with done[e] == K is frozen: the env kernel still steps it and nothing of it is
 *              recorded. Then remaining = the sum over e of K - done[e] (an integer sum: per-thread
 *              partials combined through LDS) and steps += 1.
 *   summarize  over the finished entries, flat index i = e * K + k counted iff k < done[e]. Lane j of 256
 *              takes i = j, j + 256, ... in ascending order; the 256 partials are then combined by the
 *              tree part[j] (+)= part[j + s] for s = 128, 64, ..., 1, lane j on the left. sum and sumsq
 *              are doubles of (double)returns[i], the square rounded to double before it is added (no
 *              fused multiply-add); min and max are fp32 (a < b ? a : b, the earlier partial first);
 *              length_sum and episodes are int64; unfinished = remaining. With no finished episode every
 *              field but unfinished is 0. The host restatement reduces in the same order, so the two agree
 *              bit for bit.
 *
 * One workgroup of 256 per call; no atomics; allocates nothing, does not synchronise, capturable. Every
 * pointer is device memory (mt_eval_*) or host memory (mt_eval_*_host, the same rules with no GPU; the
 * kernels are pinned against them). r_idx: [N] int32; reward, over: [N] fp32; tab_rep: [R] int32.
 * MT_ERR_ARG before any launch for a null pointer, N, K or R < 1, N * K > 2^30, or an int64 / double
 * buffer (len_acc, lengths, words, the summary) that is not 8-byte aligned. */
typedef struct mt_eval_words {
  int64_t remaining; /* episodes still owed: the sum of K - done[e] */
  int64_t steps;     /* mt_eval_step calls since the reset */
} mt_eval_words;
typedef struct mt_eval_state {
  float *ret_acc;   /* [N] */
  int64_t *len_acc; /* [N] */
  int32_t *done;    /* [N] */
  float *returns;   /* [N][K] */
  int64_t *lengths; /* [N][K] */
  mt_eval_words *words;
  int32_t N, K;
} mt_eval_state;
typedef struct mt_eval_summary {
  int64_t episodes, unfinished, length_sum;
  double sum, sumsq;
  float min, max;
  int32_t pad[2]; /* written as 0 */
} mt_eval_summary;
int mt_eval_reset(const mt_eval_state *state, mt_stream_t stream);
int mt_eval_step(const mt_eval_state *state, const int32_t *r_idx, const float *reward, const float *over,
                 const int32_t *tab_rep, int R, mt_stream_t stream);
int mt_eval_summarize(const mt_eval_state *state, mt_eval_summary *out, mt_stream_t stream);
int mt_eval_reset_host(const mt_eval_state *state);
int mt_eval_step_host(const mt_eval_state *state, const int32_t *r_idx, const float *reward, const float *over,
                      const int32_t *tab_rep, int R);
int mt_eval_summarize_host(const mt_eval_state *state, mt_eval_summary *out);

#ifdef __cplusplus
}
#endif
#endif /* MANETTE_HIP_H */
