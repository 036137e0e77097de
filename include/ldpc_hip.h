/*
 * ldpc_hip.h -- C ABI of the MI355X (gfx950) batched LDPC decode engine.
 *
 * The reference (Lalwaniamisha789/Implementation-of-Neural-LDPC-Decoders-...)
 * has no FFI or operator registry: its boundary is the Python class surface
 *     BasicMinSumDecoder.decode            ldpc_decoder.py:63-153
 *     Neural2DMinSumDecoder.forward        neural_2d_decoder.py:133-225
 *     Neural2DOffsetMinSumDecoder.forward  neural_2d_decoder.py:338-434
 *     RCQMinSumDecoder.decode              rcq_decoder.py:169-279
 *     WeightedRCQDecoder.forward           rcq_decoder.py:495-597
 * Every one of those is the same flooding loop with a different C2V rule and
 * weight lookup, so the native boundary is ONE decode entry point driven by a
 * descriptor; the Python classes of the same names (package directory) are thin
 * hosts over it.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain C types only; "device" pointers are HIP device pointers on the
 *     device that was current when the graph was created;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all
 *     work is enqueued on it, nothing synchronises, nothing allocates: the
 *     caller provides the workspace (ldpc_decoder_workspace_bytes);
 *   - handles are immutable after creation and may be shared by threads; one
 *     workspace per concurrent ldpc_decode call (two calls that may overlap on the
 *     device -- different streams, different threads -- need two workspaces);
 *   - workspaces, the `saved` block of the training path and outputs need no initialisation: no result depends on
 *     what they held before the call; every element of a non-NULL output is written, nothing beyond it is (the pad
 *     bits of a packed row, bits n .. 8 * ceil(n/8) - 1, are written as 0);
 *   - the library reads no environment variable; measurement and test hooks live in
 *     the separate ldpc_hip_debug.h and are never needed for decoding;
 *   - every function returns LDPC_OK (0) or a negative LDPC_ERR_*;
 *     ldpc_last_error() gives a thread-local message.
 */
#ifndef LDPC_HIP_H
#define LDPC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_HIP_ABI_VERSION 1

enum {
    LDPC_OK = 0,
    LDPC_ERR_ARG = -1,          /* bad argument / inconsistent descriptor        */
    LDPC_ERR_HIP = -2,          /* a HIP runtime call failed                     */
    LDPC_ERR_UNSUPPORTED = -3,  /* valid request the engine does not implement   */
    LDPC_ERR_WORKSPACE = -4     /* workspace too small                           */
};

/* arithmetic type of messages, weights, LLRs and posteriors.  LDPC_F64 takes any
 * LDPC_C2V_NMS / LDPC_C2V_OMS / LDPC_C2V_SPA table set under LDPC_SCHED_FLOODING (many
 * beta slots, per-variable alpha slots, oms_alpha) on the streaming engine; the
 * LDS-resident engine runs those of them that are LDPC_C2V_NMS with one beta slot per
 * check (any alpha table) on a code it admits, the others stream. */
enum { LDPC_F32 = 0, LDPC_F64 = 1 };

/* check-to-variable rule; `min` is min1 (min2 on the arg-min edge), `s` the
 * product of the other edges' signs with sign(0) = 0 */
enum {
    LDPC_C2V_NMS = 0,  /* c2v = (beta * min) * s             ldpc_decoder.py:118-120, neural_2d_decoder.py:189-191 */
    LDPC_C2V_RCQ = 1,  /* c2v = deq(quant((beta * s) * min)) rcq_decoder.py:242-246, 559-563 (1-byte codes in HBM) */
    LDPC_C2V_OMS = 2,  /* c2v = s * (relu(min - beta) - a_c) neural_2d_decoder.py:400-401                          */
    LDPC_C2V_SPA = 3   /* c2v = beta * 2 atanh(prod over the OTHER edges of tanh(x / 2)): sum-product / belief propagation */
};
/* LDPC_C2V_SPA is the baseline the min-sum family is measured against ("95-98 % of BP performance"); the reference has no
 * such decoder, the yardstick is a CPU restatement (tests/spa_reference.py).  Flooding schedule only.  x_e is the
 * variable-to-check message on edge e (the LLR of its variable in iteration 0) and, on the edges e of check c,
 *     c2v_e = beta_t[beta_slot[e]] * 2 atanh( prod_{e' in c, e' != e} tanh(x_e' / 2) )
 * formed by forward / backward box-plus recursions: with g(x) = log1p(exp(-x)),
 *     a [+] b = sign(a) sign(b) min(|a|, |b|) + (g(|a + b|) - g(|a - b|)),
 *     f_k = f_k-1 [+] x_k,   b_k = x_k [+] b_k+1,   c2v_k = beta * (f_k-1 [+] b_k+1)   (c2v_1 = beta * b_2, c2v_dc = beta * f_dc-1).
 * beta all 1.0 is plain BP; the tables are applied as LDPC_C2V_NMS applies them ("neural BP" weights work in the forward pass).
 * Variable update, alpha, posterior, decision (posterior < 0), syndrome, early stop, ldpc_decode_capped and packed bits are
 * those of LDPC_C2V_NMS, through the same kernels; thresholds and oms_alpha are ignored.
 *   - LLRs must be finite; finite inputs of any magnitude give finite messages.
 *   - A zero on another edge of the check gives exactly 0 (either sign).
 *   - The update is odd: negating an input negates, bit for bit, exactly the messages it feeds with odd multiplicity.
 *   - Checks of degree 0 are skipped; a graph with a check of degree 1 is refused by ldpc_decoder_create
 *     (LDPC_ERR_UNSUPPORTED: the empty product would be an infinite message).
 * fp32 and fp64; ldpc_decode, ldpc_decode_capped and (fp32) ldpc_simulate / ldpc_simulate_diag.  The engine is the two-sweep
 * streaming form: LDPC_MODE_AUTO, STREAM and SWEEPS all select it and ldpc_decoder_info reports { LDPC_MODE_SWEEPS, 0, 0, 0 };
 * RESIDENT, GATHER and PAIR are refused, as are both layered schedules, ldpc_decode_saving, ldpc_backward and every
 * ldpc_train_joint* entry point (LDPC_ERR_UNSUPPORTED). */

/* message schedule.  LAYERED_REF is RCQMinSumDecoder(layered=True) exactly as the reference runs it
 * (rcq_decoder.py:281-350): checks processed in order on running posteriors whose "previous
 * message" is never subtracted (the reference re-creates its message matrix per check); RCQ fp32 only.
 * Two kernels with identical results: LDS-resident (posteriors of a few codewords per one-wave workgroup in LDS, the lanes
 * on the edges of the current check; LDPC_MODE_AUTO / RESIDENT when a posterior vector fits LDS and no check has more than
 * 64 edges) and streaming (posteriors in HBM, a lane per codeword; LDPC_MODE_STREAM and every other case).
 * LAYERED is the schedule that code sets out to implement (and the RCQ paper defines): the check's previous
 * message IS subtracted before its update and the new one added -- an extension with no reference execution
 * to compare against (parity unpinned; checked against an independent CPU restatement only).  LAYERED applies the decoder's beta
 * table exactly as the flooding RCQ check update does (c2v = deq(quant(beta_t[beta_slot[e]] * s * min)); alpha is not used) --
 * WeightedRCQDecoder(layered="paper"); a table of all 1.0 is the unweighted schedule.  Two kernels with identical results: LDS-resident
 * (posteriors AND the per-edge message codes in LDS; LDPC_MODE_AUTO / RESIDENT when checks have <= 64 edges and at least four one-wave
 * workgroups fit a CU's LDS) and streaming (every other case).  Gradients of the RCQ form under LAYERED: ldpc_train_joint_layered_ste
 * (below) and nothing else.
 * LAYERED with LDPC_C2V_NMS / LDPC_C2V_OMS (fp32 only) is the same schedule with unquantised messages, the baseline of the quantised
 * one: on the edges of a check u = P - R, min1 / min2 / sign product over the u as in the flooding check update (first minimum is the
 * arg-min, ties keep min2 == min1, sign(0) = 0), r = (beta * min_others) * sign_others (NMS) or sign_others * (relu(min_others - beta)
 * - oms_alpha) (OMS), P = u + r, R = r; the variable-side alpha is not used, the check-side oms_alpha is; LLRs must be finite.  Two
 * kernels with identical results: LDS-resident (posteriors and a 16-byte record per check -- min1, min2, a sign and an arg-min bit per
 * edge -- from which each lane recomputes R; same qualification as above) and streaming (R as fp32 per edge in the workspace).
 * Gradients: ldpc_train_joint_layered (posterior joint training with a posterior-local gradient, below) and nothing else --
 * ldpc_decode_saving, ldpc_backward and ldpc_train_joint return LDPC_ERR_UNSUPPORTED.  LAYERED_REF with these forms is
 * unsupported (the reference has no such path), as is a float64 layered decoder.
 * LAYERED on a graph that declares layers (ldpc_graph_create_layered) has a third kernel with the same results, the
 * block-parallel one (LDPC_MODE_BLOCK): the checks of a layer share no variable, so it updates them all at once -- its dependent chain
 * per iteration is the number of layers, not the number of checks.  All three forms (NMS, OMS, RCQ weighted or not); LAYERED_REF,
 * sum-product and float64 do not have it. */
enum { LDPC_SCHED_FLOODING = 0, LDPC_SCHED_LAYERED_REF = 1, LDPC_SCHED_LAYERED = 2 };

typedef struct ldpc_graph ldpc_graph;      /* Tanner graph, CSR + CSC, device resident */
typedef struct ldpc_decoder ldpc_decoder;  /* graph + weight tables + quantiser LUTs    */

/* Replaces the reference's per-node dense scans `np.where(H[i,:]==1)` /
 * `np.where(H[:,j]==1)` (ldpc_decoder.py:92,124).  Input is the CSR edge list
 * (host memory): check i owns edges check_ptr[i]..check_ptr[i+1]-1, var_idx[e]
 * ascending inside a check.  The CSC permutation is derived inside. */
int ldpc_graph_create(ldpc_graph **out, int32_t n, int32_t m, int32_t n_edges,
                      const int32_t *check_ptr, const int32_t *var_idx);
/* ldpc_graph_create plus a partition of the checks into LAYERS: layer l is the checks layer_ptr[l] .. layer_ptr[l + 1] - 1
 * (layer_ptr [n_layers + 1] host memory, from 0 to m, strictly ascending), consecutive in CSR order and pairwise
 * variable-disjoint -- the block rows of a quasi-cyclic code, or any code after a layer ordering of its checks.  LDPC_ERR_ARG
 * for a malformed layer_ptr and for a layer two of whose checks share a variable (the message names the layer and the
 * variable).  The graph decodes exactly as one made by ldpc_graph_create under every mode that exists there; the layers
 * are read by LDPC_MODE_BLOCK only. */
int ldpc_graph_create_layered(ldpc_graph **out, int32_t n, int32_t m, int32_t n_edges,
                              const int32_t *check_ptr, const int32_t *var_idx,
                              int32_t n_layers, const int32_t *layer_ptr);
/* *n_layers = the number of declared layers (0: created without); layer_ptr_out: NULL or room for n_layers + 1 entries */
int ldpc_graph_layers(const ldpc_graph *g, int32_t *n_layers, int32_t *layer_ptr_out);
void ldpc_graph_destroy(ldpc_graph *g);
/* n, m, E, max check degree, max variable degree */
int ldpc_graph_info(const ldpc_graph *g, int32_t out5[5]);

/* All pointers are HOST pointers, copied at creation.  Weight tables are
 * dtype-typed ([iters][slots], row t = iteration t); slot arrays say which
 * table column an edge / a variable uses -- the flattened form of
 * _get_beta_weight/_get_alpha_weight (neural_2d_decoder.py:84-131). */
typedef struct {
    int32_t dtype;              /* LDPC_F32 | LDPC_F64                                     */
    int32_t c2v_form;           /* LDPC_C2V_*                                              */
    int32_t iters;              /* T = max_iterations                                      */
    int32_t n_beta_slots;
    const void *beta;           /* [T][n_beta_slots]                                       */
    const int32_t *beta_slot;   /* [E] per CSR edge                                        */
    int32_t n_alpha_slots;
    const void *alpha;          /* [T][n_alpha_slots]  V2C weight: llr + alpha * sum       */
    const int32_t *alpha_slot;  /* [n] per variable                                        */
    /* RCQ only: NonUniformQuantizer tables (rcq_decoder.py:48-57) as float32(tau)  */
    int32_t n_levels;           /* 2^(bc-1), <= 128                                        */
    int32_t n_quantizers;
    const float *thresholds;    /* [n_quantizers][n_levels]                                */
    const int32_t *q_of_iter;   /* [T] quantiser used in iteration t (rcq_decoder.py:156-167) */
    /* OMS only: check-side offset alpha (neural_2d_decoder.py:392,400)              */
    int32_t n_oms_alpha_slots;
    const void *oms_alpha;      /* [T][n_oms_alpha_slots] or NULL (= 0)                    */
    const int32_t *oms_alpha_slot; /* [E]                                                  */
    int32_t schedule;           /* LDPC_SCHED_FLOODING (0) | LDPC_SCHED_LAYERED_REF | LDPC_SCHED_LAYERED */
} ldpc_decoder_desc;

int ldpc_decoder_create(ldpc_decoder **out, const ldpc_graph *g, const ldpc_decoder_desc *desc);

/* Two engines implement the same arithmetic (bit-identical results):
 *   STREAM   : messages in HBM ([tile][edge][W]); any code, fp32/fp64.  One kernel per sweep (check sweep,
 *              variable sweep).  fp32 flooding RCQ decoders have two cheaper forms, STREAM takes the first that applies:
 *                PAIR   -- one beta per check, sorted thresholds, <= 62 levels: both message directions are 1-byte
 *                          codes (the variable sweep quantises with the next iteration's beta and thresholds, the
 *                          check sweep is integer-only): 4E + 4n bytes per codeword and iteration;
 *                GATHER -- variable degree <= 8: ONE fused kernel per iteration that recomputes the variable->check
 *                          messages from the 1-byte check->variable codes and the LLRs (no V2C array);
 *              SWEEPS forces the plain two-sweep form (fp32 V2C rows); GATHER / PAIR force that form (error when the
 *              decoder does not qualify).
 *              On fp32 256-codeword tiles the last variable pass writes the caller's posterior / decision rows itself, and the
 *              PAIR form's entrance pass also codes the LLRs for iteration 0 (no separate layout passes at either end).
 *   RESIDENT : one fused kernel, messages in LDS for all T iterations; fp32 codes with
 *              dv <= 8 whose state fits 160 KiB of LDS (e.g. the (1998,1512) code); for the layered schedule: the
 *              LDS-resident layered kernel (see LDPC_SCHED_LAYERED_REF)
 *   BLOCK    : the block-parallel layered kernel: LDPC_SCHED_LAYERED, fp32, on a graph created with layers
 *              (ldpc_graph_create_layered) whose checks have at most 64 edges and whose per-codeword state (posteriors and
 *              check records or message codes) fits LDS.  G codewords per workgroup in LDS, a thread per check of the current
 *              layer and codeword, one barrier per layer.  LDPC_ERR_UNSUPPORTED, with the reason, for a graph without layers,
 *              a float64 decoder, another schedule and a state that does not fit.  RESIDENT keeps meaning the sequential
 *              LDS kernels and STREAM the streaming walk on such a graph too.
 * AUTO (default) takes RESIDENT when the code qualifies, else STREAM.  AUTO never takes BLOCK: measured, it wins from a mean
 * layer size of 16 on quasi-cyclic codes (5x at Z = 81) but loses on a layer-ordered irregular code at 24, so no threshold on
 * the layer size alone is safe yet (DESIGN.md 3f'); ask for it with LDPC_MODE_BLOCK. */
enum { LDPC_MODE_AUTO = 0, LDPC_MODE_STREAM = 1, LDPC_MODE_RESIDENT = 2, LDPC_MODE_SWEEPS = 3, LDPC_MODE_GATHER = 4,
       LDPC_MODE_PAIR = 5, LDPC_MODE_BLOCK = 6 };
int ldpc_decoder_set_mode(ldpc_decoder *d, int32_t mode);
/* out4 = { engine and form a decode would use now (LDPC_MODE_RESIDENT, LDPC_MODE_BLOCK, or the streaming form LDPC_MODE_PAIR /
 * LDPC_MODE_GATHER / LDPC_MODE_SWEEPS), codewords per workgroup, threads per
 * workgroup, LDS bytes per workgroup } -- the last three 0 when the code does not qualify; the geometry of a
 * fixed-iteration decode where it has one of its own (the compact resident kernel) */
int ldpc_decoder_info(const ldpc_decoder *d, int32_t out4[4]);
/* re-upload beta/alpha(/oms_alpha) tables of an existing decoder (same shapes);
 * enqueued on `stream`, host arrays must stay valid until it has run. */
int ldpc_decoder_set_weights(ldpc_decoder *d, const void *beta, const void *alpha,
                             const void *oms_alpha, void *stream);
/* replace the quantiser tables of an LDPC_C2V_RCQ decoder: thresholds is host [n_quantizers][n_levels] fp32, the shapes the
 * decoder was created with (LDPC_ERR_UNSUPPORTED for a decoder of another form).  Contract of ldpc_decoder_set_weights:
 * the uploads (threshold table, signed reconstruction LUT) are enqueued on `stream`, `thresholds` must stay valid until it has
 * run, and the next call must not be made before.  Everything ldpc_decoder_create derives from the threshold VALUES is
 * derived again -- which streaming form applies (code pair / its float key), the resident kernels' tau_0 == 0 shortcut and
 * the compact plan's check words, the layered kernels' lean instantiation -- so every decode and training call afterwards
 * equals that of a decoder created with these tables, bit for bit; nothing of the graph, the plans' layout or the weights
 * is rebuilt.  When the mode was forced to LDPC_MODE_PAIR and the new table does not admit that form (thresholds 1.. not
 * positive and sorted) the call returns LDPC_ERR_UNSUPPORTED and leaves the decoder exactly as it was. */
int ldpc_decoder_set_quantizers(ldpc_decoder *d, const float *thresholds, void *stream);
void ldpc_decoder_destroy(ldpc_decoder *d);

/* bytes of device scratch ldpc_decode needs for a batch of `batch` codewords */
size_t ldpc_decoder_workspace_bytes(const ldpc_decoder *d, int64_t batch);

/* Decode llr[batch][n] (device, row-major, dtype of the decoder).
 *   early_stop != 0 : reference semantics per codeword -- outputs are those of the
 *                     first iteration whose syndrome is zero (iterations 1-based,
 *                     success 1), else of iteration T (success 0);
 *   early_stop == 0 : exactly T iterations; success = final syndrome is zero.
 * Outputs (device, any may be NULL):
 *   bits[batch][n] int32 (posterior < 0), posterior[batch][n] dtype,
 *   iterations[batch] int32, success[batch] uint8,
 *   packed_bits[batch][ceil(n/8)] uint8, bit j of a codeword at byte j/8, bit j%8
 *   (wire format of the multi-GPU all-gather).
 * Rows: any n >= 1, rows packed (row b starts n elements after row b - 1).  llr, posterior and bits each need only
 * the alignment of their element type -- 4 bytes for llr / posterior of an fp32 decoder and for bits, 8 bytes for
 * llr / posterior of an fp64 decoder -- and are independent of one another: wider alignment (up to 16 bytes, of the
 * pointer and of the row length in bytes) is used where present and never required, and no result depends on it
 * (tests/test_gpu_row_alignment.py).  The same holds for ldpc_decode_capped and ldpc_decode_saving. */
int ldpc_decode(const ldpc_decoder *d, const void *llr, int64_t batch, int32_t early_stop,
                int32_t *bits, void *posterior, int32_t *iterations, uint8_t *success,
                uint8_t *packed_bits, void *workspace, size_t workspace_bytes, void *stream);

/* ldpc_decode with at most `max_iterations` (>= 1) of the decoder's iterations: iteration t still uses the decoder's own
 * tables of iteration t (weights, quantiser schedule), a codeword open at the cap reports iterations = cap, success = 0.
 * No reference counterpart: it lets a batched caller with early stop (the Monte-Carlo driver, simulation_framework.py:85-139
 * of the reference run block-wise) decode a block up to the iteration by which most codewords have stopped and finish the few
 * stragglers as a small second batch -- the streaming engine freezes whole 256-codeword tiles only. */
int ldpc_decode_capped(const ldpc_decoder *d, const void *llr, int64_t batch, int32_t early_stop,
                       int32_t max_iterations, int32_t *bits, void *posterior, int32_t *iterations,
                       uint8_t *success, uint8_t *packed_bits, void *workspace, size_t workspace_bytes,
                       void *stream);

/* ---- gradient (training) path -------------------------------------------------------------
 * Replaces torch autograd through Neural2DMinSumDecoder.forward / NeuralMinSumDecoder.forward
 * (neural_2d_decoder.py:133-225 under loss.backward(), training_framework.py:127-134): the
 * derivative of any loss of the returned posterior with respect to the beta / alpha tables.
 * fp32 LDPC_C2V_NMS and LDPC_C2V_OMS flooding decoders (LDPC_ERR_UNSUPPORTED otherwise; the reference's
 * RCQ quantiser passes no gradient).  Always runs the streaming engine.
 *
 * ldpc_decode_saving : ldpc_decode (same outputs, same arithmetic) that also keeps every
 *   iteration's message rows in `saved` (ldpc_train_saved_bytes: (2T-1) * E * 4 bytes per
 *   codeword, tile-padded).
 * ldpc_backward      : grad_posterior[batch][n] fp32 (d loss / d posterior) and the
 *   iterations[batch] that decode returned -> grad_beta[T][n_beta_slots], grad_alpha[T][n_alpha_slots]
 *   fp32 and, for LDPC_C2V_OMS decoders created with oms_alpha, grad_oms_alpha[T][n_oms_alpha_slots]
 *   and grad_llr[batch][n] fp32 (d loss / d llr, for callers that train what produces the LLRs)
 *   (device, overwritten; any may be NULL).  The decoder's tables must be the ones the
 *   forward call used.  Slots autograd would leave without a gradient come back as 0.
 * Both need ldpc_train_workspace_bytes of 256-byte aligned scratch; `saved` is 256-byte aligned. */
size_t ldpc_train_saved_bytes(const ldpc_decoder *d, int64_t batch);
size_t ldpc_train_workspace_bytes(const ldpc_decoder *d, int64_t batch);
int ldpc_decode_saving(const ldpc_decoder *d, const void *llr, int64_t batch, int32_t early_stop,
                       int32_t *bits, void *posterior, int32_t *iterations, uint8_t *success,
                       void *saved, size_t saved_bytes, void *workspace, size_t workspace_bytes,
                       void *stream);
int ldpc_backward(const ldpc_decoder *d, const void *saved, size_t saved_bytes, const void *llr,
                  int64_t batch, const int32_t *iterations, const void *grad_posterior,
                  void *grad_beta, void *grad_alpha, void *grad_oms_alpha, void *grad_llr,
                  void *workspace, size_t workspace_bytes, void *stream);


/* ---- posterior joint training (the paper's training method) -------------------------------
 * The fixed-T decode (no early stop) of the same fp32 LDPC_C2V_NMS / LDPC_C2V_OMS flooding decoders
 * (LDPC_ERR_UNSUPPORTED otherwise, as ldpc_decode_saving) with the loss taken on the posterior
 * l_t of EVERY iteration t = 0..T-1:
 *   J_t = mean over b, j of BCEWithLogits(-l_t[b][j], targets[b][j])      J = sum_t w_t * J_t
 * and the gradient of J with the previous iteration's leave-one-out C2V sum in the variable update
 * treated as a constant, so iteration t's loss reaches beta_t, the offset alpha_t, alpha_t-1 (through
 * v2c_t) and the LLRs, nothing earlier.  The gradients are formed while iteration t is decoded: the
 * scratch (ldpc_train_joint_workspace_bytes, 256-byte aligned) does not depend on T and nothing is saved.
 *   llr[batch][n], targets[batch][n] (NULL: all zero), iteration_weights[T] fp32 (device; read only when
 *   a gradient is asked for) -> loss_per_iter[T] = J_t fp32, bits[batch][n] int32 and posterior[batch][n]
 *   fp32 of the last iteration (identical to ldpc_decode with early_stop = 0), grad_beta[T][n_beta_slots],
 *   grad_alpha[T][n_alpha_slots], grad_oms_alpha[T][n_oms_alpha_slots], grad_llr[batch][n] fp32 (device,
 *   overwritten; bits, posterior and every gradient may be NULL -- with no gradient only the loss is
 *   formed).  Parameters the loss cannot reach (alpha_T-1, the alpha table of the offset forms) get 0;
 *   batch == 0 gives zero losses and gradients.  Deterministic: no atomics. */
size_t ldpc_train_joint_workspace_bytes(const ldpc_decoder *d, int64_t batch);
int ldpc_train_joint(const ldpc_decoder *d, const void *llr, const void *targets, int64_t batch,
                     const void *iteration_weights, void *loss_per_iter, int32_t *bits, void *posterior,
                     void *grad_beta, void *grad_alpha, void *grad_oms_alpha, void *grad_llr,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---- posterior joint training of the quantised decoder (straight-through estimator) ----------
 * ldpc_train_joint for the fp32 LDPC_C2V_RCQ flooding decoders (LDPC_ERR_UNSUPPORTED for every other decoder;
 * ldpc_train_joint itself keeps refusing these).  Same loss, same outputs, same empty-batch / NULL-output /
 * alignment rules, no grad_oms_alpha; scratch ldpc_train_joint_ste_workspace_bytes (the C2V rows it keeps are 1-byte codes).
 *   Forward : the decoder's own fixed-T two-sweep decode, unchanged -- bits, posterior and every iteration's posterior l_t
 *             equal ldpc_decode / ldpc_decode_capped with early_stop = 0 bit for bit.
 *   Gradient: posterior-local as above (J_t reaches beta_t, alpha_t-1 and the LLRs; alpha_T-1 gets 0), with the quantiser
 *             differentiated by the straight-through rule.  With m = beta_t[slot(e)] * s * min the value the forward
 *             quantises (min / min2 / first-index arg-min / sign(0) = 0 / degree-1 rules and second-minimum tie split of
 *             the LDPC_C2V_NMS backward), code_t[e] the code the forward wrote and L = n_levels:
 *                 c2v_t[e]          = deq_t(code_t[e])                         (value, exact)
 *                 d c2v_t[e] / d m := 1  if (code_t[e] mod L) < L - 1          (below the top level, dead zone included)
 *                                     0  otherwise                             (saturated)
 *             The mask is a function of the code the forward stored, not of a repeated comparison.  The constants of the
 *             alpha_t-1 partial are leave-one-out sums of deq_t-1(code_t-1[.]): the quantiser of iteration t-1
 *             (q_of_iter[t-1]), not of iteration t.
 * Deterministic: no atomics. */
size_t ldpc_train_joint_ste_workspace_bytes(const ldpc_decoder *d, int64_t batch);
int ldpc_train_joint_ste(const ldpc_decoder *d, const void *llr, const void *targets, int64_t batch,
                         const void *iteration_weights, void *loss_per_iter, int32_t *bits, void *posterior,
                         void *grad_beta, void *grad_alpha, void *grad_llr,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ---- posterior joint training of the layered min-sum decoders -----------------------------------
 * ldpc_train_joint for the fp32 LDPC_SCHED_LAYERED decoders of LDPC_C2V_NMS / LDPC_C2V_OMS.  LDPC_ERR_UNSUPPORTED for every
 * other decoder, with a message naming the entry point to take: flooding min-sum -> ldpc_train_joint, flooding RCQ ->
 * ldpc_train_joint_ste, LAYERED RCQ -> ldpc_train_joint_layered_ste; LAYERED_REF and float64 have none.  ldpc_train_joint itself keeps
 * refusing layered decoders.  Same outputs, same empty-batch / NULL-output / alignment / T < 1 / no-edges rules; scratch
 * ldpc_train_joint_layered_workspace_bytes (256-byte aligned, independent of T).  An extension like the schedule: nothing in
 * the reference executes it, the yardstick is a CPU restatement.
 *   Forward : the decoder's own fixed-T layered decode, no early stop, one iteration per kernel launch with posteriors and
 *             messages kept in the scratch -- bits and posterior equal ldpc_decode(early_stop = 0) bit for bit, and the
 *             posterior P_t after the last check of iteration t equals ldpc_decode_capped(max_iterations = t + 1,
 *             early_stop = 0) bit for bit.
 *   Loss    : J_t = mean over b, j of BCEWithLogits(-P_t[b][j], targets[b][j]),  J = sum_t w_t * J_t, with the seed
 *             g_t = w_t * (y - sigmoid(-P_t)) / (B n), as ldpc_train_joint.
 *   Gradient (layered posterior-local): when check i is processed in iteration t each of its edges e = (i, v) has
 *             u_e = P_v - R_e.  Write u_e = llr_v + x_e: x_e, the sum of the variable's other messages (new and old), is a
 *             constant, and the posterior is taken as P_t[v] = llr_v + sum over the edges e at v of r_t,e.  So J_t reaches
 *             beta_t, the offset form's oms_alpha_t and the LLRs -- nothing earlier, and nothing through another check of
 *             the same iteration.  The derivatives of r are those of the flooding check update with v2c_t := u:
 *                 NMS  d r_e/d beta = raw_e * prod_e                d r_e/d raw_e = beta * prod_e
 *                 OMS  d r_e/d beta = -prod_e * [raw_e - beta > 0]  d r_e/d a = -prod_e  d r_e/d raw_e = prod_e * [raw_e - beta > 0]
 *             prod_e = 0 when another edge of the check has u == 0 exactly (a degree-1 check: prod = 1, min2 = min1);
 *             d|x| = sgn(x), sgn(0) = 0; the minimum's gradient goes to the first arg-min edge, the second minimum's is
 *             split evenly over the edges tied for it.
 *                 d J/d llr_v = sum_t ( g_t[v] + sum over the edges e at v of d J_t/d u_e )
 *             The variable-side alpha is not used by the schedule: grad_alpha, when given, is zero-filled [T][n_alpha_slots].
 * Deterministic: no atomics. */
size_t ldpc_train_joint_layered_workspace_bytes(const ldpc_decoder *d, int64_t batch);
int ldpc_train_joint_layered(const ldpc_decoder *d, const void *llr, const void *targets, int64_t batch,
                             const void *iteration_weights, void *loss_per_iter, int32_t *bits, void *posterior,
                             void *grad_beta, void *grad_alpha, void *grad_oms_alpha, void *grad_llr,
                             void *workspace, size_t workspace_bytes, void *stream);

/* ---- posterior joint training of the layered quantised decoder (straight-through estimator) -----
 * ldpc_train_joint_ste for the fp32 LDPC_C2V_RCQ decoders under LDPC_SCHED_LAYERED (WeightedRCQDecoder(layered="paper")).
 * LDPC_ERR_UNSUPPORTED for every other decoder, with a message naming the entry point to take: flooding RCQ ->
 * ldpc_train_joint_ste, layered min-sum -> ldpc_train_joint_layered, flooding min-sum -> ldpc_train_joint; LAYERED_REF and
 * float64 have none.  The other three entry points keep refusing this decoder.  Argument list and rules of
 * ldpc_train_joint_ste (empty batch, NULL outputs, alignment, no grad_oms_alpha); scratch
 * ldpc_train_joint_layered_ste_workspace_bytes: (2E + 4n) * 4 + E bytes per codeword of the 64-codeword tiles plus per-tile
 * partials, independent of T.  A definition: nothing in the reference executes it, the yardstick is a CPU restatement.
 *   Forward : the decoder's own fixed-T LAYERED decode, no early stop, one iteration per kernel launch with the posteriors
 *             and the 1-byte message codes kept in the scratch.  In iteration t, on the edges e = (c, v) of check c:
 *             u_e = P_v - deq_t'(code_e), t' the iteration that wrote the code (its quantiser is q_of_iter[t-1]; nothing is
 *             subtracted in iteration 0); min1 / min2 / sign product over the u as in the flooding RCQ check update;
 *             m_e = +-(beta_t[beta_slot[e]] * raw_e), the product rounded before the sign; code_e = quant_t(m_e) =
 *             (m_e < 0) * L + level, r_e = deq_t(code_e), P_v = u_e + r_e.  bits and posterior equal
 *             ldpc_decode(early_stop = 0) bit for bit, and the posterior P_t after the last check of iteration t equals
 *             ldpc_decode_capped(max_iterations = t + 1, early_stop = 0) bit for bit, on either decode kernel.
 *   Loss    : that of ldpc_train_joint on P_t, with the seed g_t = w_t * (y - sigmoid(-P_t)) / (B n).
 *   Gradient: the layered posterior-local rule of ldpc_train_joint_layered composed with the straight-through rule of
 *             ldpc_train_joint_ste.  P_t[v] = llr_v + sum over the edges e at v of r_t,e;  u_e = llr_v + x_e, x_e a constant;
 *                 d r_e / d m_e := 1  if (code_t[e] mod L) < L - 1      (below the top level, dead zone included)
 *                                  0  otherwise                         (saturated)
 *             with the mask read from the code the walk stored, and m_e differentiated in beta_t and in the |u| of the
 *             check's other edges by the rules of the flooding RCQ backward (first-index arg-min, a tied second minimum
 *             split evenly, sgn(0) = 0 and a zero product when another edge is exactly 0, degree 1: product 1 and
 *             min2 = min1).  J_t reaches beta_t and the LLRs through the one check update that wrote each message -- nothing
 *             earlier, nothing through another check of the same iteration:
 *                 d J/d llr_v = sum_t ( g_t[v] + sum over the edges e at v of d J_t/d u_e )
 *             alpha is not used by the schedule: grad_alpha, when given, is zero-filled [T][n_alpha_slots].
 * Deterministic: no atomics. */
size_t ldpc_train_joint_layered_ste_workspace_bytes(const ldpc_decoder *d, int64_t batch);
int ldpc_train_joint_layered_ste(const ldpc_decoder *d, const void *llr, const void *targets, int64_t batch,
                                 const void *iteration_weights, void *loss_per_iter, int32_t *bits, void *posterior,
                                 void *grad_beta, void *grad_alpha, void *grad_llr,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* ---- level gradients of the quantised joint losses (learned quantisers) -----------------------------
 * ldpc_train_joint_ste and ldpc_train_joint_layered_ste with one more output: the gradient of J with respect to the
 * RECONSTRUCTION values of the quantiser.  Argument lists, rules, refusals and error messages of the entry point each
 * extends; every other output is bit-identical to that entry point's; scratch from the ..._levels_workspace_bytes function
 * of its own (the base layout followed by the per-wave partials).  L = n_levels.
 *   grad_levels[T][L] fp32 (device, overwritten, may be NULL: then exactly the launches of the base entry point):
 *       grad_levels[t][l] = sum over b < batch and the edges e of [code_t[b][e] mod L == l] * s(code_t[b][e]) * g_t[b][var(e)]
 *   with code_t the byte the forward stored for the edge in iteration t, s = +1 for code < L and -1 otherwise, and
 *   g_t = w_t * (y - sigmoid(-l_t)) / (B n) the seed of J_t.  It is d J_t / d tau_l under the rule both entry points use:
 *   l_t[v] = llr_v + sum over the edges at v of deq_t(code_t[e]) (layered: P_t[v] = llr_v + sum of r_t,e), deq of level l is
 *   +-tau_l, the thresholds as decision boundaries get no gradient (straight-through: the codes are what the forward
 *   stored) and the leave-one-out sums of the next variable update stay constants.  Level 0 and the top level get a
 *   gradient like any other; a saturated message, which passes nothing to beta, still moves tau_L-1.  Row t belongs to the
 *   quantiser q_of_iter[t]; summing rows per quantiser and the chain rule to whatever parametrises tau are the caller's.
 *   Codewords b >= batch of the last tile contribute nothing whatever the scratch held; batch == 0 gives zeros.
 *   Summation: fp32 within one wave's chunk of 64 edges, fp64 above (lanes, waves, tiles in a fixed order), rounded once.
 * Deterministic: no atomics. */
size_t ldpc_train_joint_ste_levels_workspace_bytes(const ldpc_decoder *d, int64_t batch);
int ldpc_train_joint_ste_levels(const ldpc_decoder *d, const void *llr, const void *targets, int64_t batch,
                                const void *iteration_weights, void *loss_per_iter, int32_t *bits, void *posterior,
                                void *grad_beta, void *grad_alpha, void *grad_llr, void *grad_levels,
                                void *workspace, size_t workspace_bytes, void *stream);
size_t ldpc_train_joint_layered_ste_levels_workspace_bytes(const ldpc_decoder *d, int64_t batch);
int ldpc_train_joint_layered_ste_levels(const ldpc_decoder *d, const void *llr, const void *targets, int64_t batch,
                                        const void *iteration_weights, void *loss_per_iter, int32_t *bits, void *posterior,
                                        void *grad_beta, void *grad_alpha, void *grad_llr, void *grad_levels,
                                        void *workspace, size_t workspace_bytes, void *stream);

/* ---- on-device Monte-Carlo (BI-AWGN) ---------------------------------------------------------
 * The reference's deliverable is FER / BER curves (simulation_framework.py:85-139: draw, decode, count, stop at max_frames
 * frames or max_errors frame errors).  These entry points keep a whole SNR point on the device.
 *
 * ldpc_channel_awgn : llr[batch][n] fp32 (device, 4-byte aligned, row-major) of frames first_frame .. first_frame + batch - 1
 *   from a counter-based stream -- frame f gets the same noise whatever block it is drawn in, on whatever device.  Needs no
 *   decoder; asynchronous on `stream`.  Sample j of frame f:
 *     (x0, x1, x2, x3) = Philox4x32-10(counter = (f & 0xffffffff, f >> 32, j / 4, stream_id),
 *                                      key = (seed & 0xffffffff, seed >> 32))
 *       multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds;
 *     u(x) = fmaf((float)x, 0x1p-32f, 0x1p-33f)   in (0, 1]; the uint -> float conversion rounds to nearest;
 *     r = sqrtf(-2.0f * logf(u(x0))), theta = 6.2831853071795865f * u(x1), z[4q] = r * cosf(theta), z[4q+1] = r * sinf(theta),
 *     (x2, x3) give z[4q+2] and z[4q+3] the same way (accurate fp32 log / sincos / sqrt, no fast-math);
 *     llr[b][j] = s_j * fmaf(z, scale, shift),  s_j = +1 for codeword bit 0, -1 for bit 1 (codeword_packed: device,
 *     ceil(n/8) bytes, bit j at byte j/8, bit j%8; NULL = all-zero codeword).
 *   The smallest uniform is 2^-33: the tails of the normal reach +-6.76 sigma and no further.  Symbol and noise flip together,
 *   so a nonzero codeword's LLRs are the exact sign mirror of the all-zero draw.  scale = 2/sigma and shift = 2/sigma^2 are
 *   computed by the caller in double and passed as fp32; the reference's literal channel (bit 0 -> -1) passes -shift.
 *
 * ldpc_channel_awgn_mix : the same stream with the SNR point a function of the frame (mixed-SNR training batches).  Sample j
 *   of frame f uses exactly the counter, key, uniforms and Box-Muller above -- the normal z of a frame does not depend on which
 *   of the two entry points draws it -- and
 *     llr[b][j] = s_j * fmaf(z, scale_tab[p], shift_tab[p]),  p = f mod n_points,  f = first_frame + b (64-bit, absolute).
 *   The point is a property of the frame, not of the block: any run of at least n_points consecutive frames holds every point
 *   in equal share, up to one frame, however the stream is cut into blocks.  n_points == 1 is
 *   ldpc_channel_awgn(scale_tab[0], shift_tab[0]) bit for bit.  scale_tab / shift_tab: device fp32, 4-byte aligned, n_points
 *   entries each, read only, computed by the caller in double (negative shifts for the reference's literal channel);
 *   codeword_packed as above.  LDPC_ERR_ARG, in this order, for batch < 0, batch > 2^31 - 1, n < 1, n_points outside
 *   1 .. 4096, and a block that would wrap the 64-bit frame index (first_frame > 2^64 - batch: p is not continuous across the
 *   wrap); then batch == 0 returns LDPC_OK without touching a pointer; then a NULL or misaligned llr, NULL or misaligned
 *   tables.  The two limits keep the point index of a lane in 32-bit arithmetic.  Asynchronous on `stream`, allocates nothing,
 *   safe under stream capture, like ldpc_channel_awgn.
 *
 * ldpc_sim_count : folds one decoded block -- packed_bits[batch][ceil(n/8)] and iterations[batch] as ldpc_decode writes them --
 *   into state[8] (device, int64) = { frames, frame_errors, bit_errors, iterations, done, blocks_seen, 0, 0 }; the caller
 *   zeroes the state to start a point.  Per frame wrong = popcount(packed XOR codeword) over bits < n (pad bits of the last
 *   byte are ignored), a frame error when wrong > 0.  Frames are consumed IN ORDER, as the reference's loop does: at most
 *   max_frames - frames of them, and none after the frame at which frame_errors reaches max_errors; the frame errors, wrong
 *   bits and iterations of the consumed frames are added.  done is set once frames >= max_frames or frame_errors >= max_errors;
 *   a launch that finds done set changes nothing but blocks_seen.  The last two words are scratch between the two kernels of
 *   a call and zero again after it.  Asynchronous on `stream`; calls on one state must be ordered by the stream.
 *
 * ldpc_simulate : one SNR point with an fp32 decoder of any schedule and engine (float64: LDPC_ERR_UNSUPPORTED).  Block k is
 *   frames first_frame + k * block .. of the stream above (the last block of a point min(block, max_frames - frames drawn)
 *   frames): channel, ldpc_decode(early_stop = 1) with packed decisions and iterations only, ldpc_sim_count, all inside
 *   `workspace` (ldpc_simulate_workspace_bytes, 256-byte aligned) with nothing synchronised in between.  Every poll_blocks
 *   blocks the state is copied to pinned host memory and the stream synchronised; the call returns once done is set, with the
 *   state in out_state (host).  Blocks queued after the point finished are no-ops in the counter, so the first five words of
 *   the result do not depend on block or poll_blocks (blocks_seen does).  UNLIKE every other entry point this one is
 *   SYNCHRONOUS, allocates (64 bytes of pinned host memory per call) and must NOT be called during stream capture.
 *
 * Diagnostics.  ldpc_sim_count_diag is ldpc_sim_count -- the same eight state words for the same block, `done` and
 *   blocks_seen included -- that also keeps a diag buffer (device, int64 words, 8-byte aligned, ldpc_sim_diag_words(T, capture)
 *   of them, zeroed by the caller to start a point) over the CONSUMED frames, with `success` as ldpc_decode writes it:
 *     diag[0]             undetected frame errors: wrong > 0 and success != 0 (the decisions satisfy H and are not the codeword)
 *     diag[1]             records written = min(frame errors consumed so far, capture)
 *     diag[2], diag[3]    0 (diag[2] is scratch between the two kernels of a call and zero again after it)
 *     diag[4 + t]         t = 0 .. T: consumed frames with iterations == t (iterations clamped to [0, T])
 *     diag[5 + T + 4k ..] record k = { absolute frame index block_first_frame + row, wrong bits, iterations, undetected 0/1 }
 *   Records are the first `capture` frame errors the point consumes, in frame order; none is written for a frame the stop rule
 *   does not consume.  Everything is defined on the ordered stream of frames, so nothing in state or diag depends on how the
 *   point is cut into blocks.  A launch that finds done set changes nothing but blocks_seen.  The frame index is all a failure
 *   needs: ldpc_channel_awgn(batch = 1, first_frame = record[0]) with the point's seed, stream_id, scale, shift and codeword
 *   draws that frame again, bit for bit.  T is the decoder's iteration count (any T >= 0; the histogram has T + 1 bins) and
 *   capture >= 0; both must not change during a point.  scratch: device, 4-byte aligned, ldpc_sim_count_diag_scratch_bytes(batch)
 *   (4 bytes per frame); NULL success / diag / scratch are accepted only with batch == 0.
 * ldpc_simulate_diag is ldpc_simulate with a success row, the scratch and the diag buffer carved into its workspace
 *   (ldpc_simulate_diag_workspace_bytes); it returns the diag buffer in out_diag (host, ldpc_sim_diag_words(T of d, capture)
 *   words) with the final state.  The first five state words equal ldpc_simulate's.  Synchronous, as ldpc_simulate. */
typedef struct {
    uint64_t seed;
    uint32_t stream_id;
    uint64_t first_frame;
    float scale, shift;
    const uint8_t *codeword_packed;   /* device, or NULL: all-zero codeword */
    int64_t max_frames, max_errors;
    int64_t block;                    /* frames per block, >= 1 */
    int32_t poll_blocks;              /* blocks between two looks at the state, >= 1 */
} ldpc_sim_desc;

int ldpc_channel_awgn(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                      float scale, float shift, const uint8_t *codeword_packed, void *stream);
int ldpc_channel_awgn_mix(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                          const float *scale_tab, const float *shift_tab, int32_t n_points,
                          const uint8_t *codeword_packed, void *stream);
int ldpc_sim_count(int64_t *state, const uint8_t *packed_bits, const int32_t *iterations, int64_t batch, int32_t n,
                   const uint8_t *codeword_packed, int64_t max_frames, int64_t max_errors, void *stream);
size_t ldpc_simulate_workspace_bytes(const ldpc_decoder *d, int64_t block);
int ldpc_simulate(const ldpc_decoder *d, const ldpc_sim_desc *desc, int64_t out_state[8], void *workspace,
                  size_t workspace_bytes, void *stream);

/* words of a diag buffer: 4 header words, T + 1 histogram bins, 4 words per captured frame (0: T < 0 or capture < 0) */
size_t ldpc_sim_diag_words(int32_t T, int64_t capture);
size_t ldpc_sim_count_diag_scratch_bytes(int64_t batch);
int ldpc_sim_count_diag(int64_t *state, int64_t *diag, int32_t T, int64_t capture,
                        const uint8_t *packed_bits, const int32_t *iterations, const uint8_t *success,
                        int64_t batch, int32_t n, const uint8_t *codeword_packed, uint64_t block_first_frame,
                        int64_t max_frames, int64_t max_errors, void *scratch, size_t scratch_bytes, void *stream);
size_t ldpc_simulate_diag_workspace_bytes(const ldpc_decoder *d, int64_t block, int64_t capture);
int ldpc_simulate_diag(const ldpc_decoder *d, const ldpc_sim_desc *desc, int64_t capture, int64_t out_state[8],
                       int64_t *out_diag /* host, ldpc_sim_diag_words(T of d, capture) */,
                       void *workspace, size_t workspace_bytes, void *stream);

/* ---- rate matching: punctured and shortened bits on the channel, a count mask on the counters ----
 * A profile says which of the n variable nodes were not sent (punctured), which are known to the receiver (shortened) and
 * which bits the error counters look at.  Each _rm entry point is the entry point above with `const ldpc_rate_match *rm`
 * inserted before `stream` (after `desc` for the two simulate forms); rm == NULL is the plain call and launches the very same
 * kernels.  The struct lives on the host, its masks on the device; ldpc_sim_desc and the workspace sizes are unchanged.
 *
 * Channel.  Sample j of frame f draws exactly the normal z that ldpc_channel_awgn defines -- the Philox counter is on the
 * VARIABLE index j, not on the transmit position -- so a rate-matched draw equals the plain draw on every transmitted
 * position, bit for bit, and the profiles of a rate-compatible family are compared on common noise.  Then
 *     punctured bit      llr = +0.0f (positive zero whatever the codeword bit is: an erasure, sign(0) = 0 in the min-sum kernels)
 *     shortened bit      llr = s_j * short_llr
 *     bit in both masks  shortened
 * Bits at and beyond n in a mask's last byte are ignored.  LDPC_ERR_ARG when shortened_packed is given and short_llr is not
 * finite and > 0; that check comes after the scalar argument checks of the plain call and before batch == 0 returns LDPC_OK
 * without touching a device pointer; the pointer checks follow in the order of the plain call.
 *
 * Counters.  wrong = popcount((packed XOR codeword) AND count_packed) over bits < n takes the place of `wrong` everywhere: a
 * frame error is wrong > 0, the stop rule runs on it, "undetected" is wrong > 0 with success != 0, the records hold it.  state,
 * diag, done and blocks_seen are those of the plain counters; count_packed == NULL gives the plain counters' words exactly.
 * Only count_packed is read by the two counter calls.
 *
 * ldpc_simulate_rm / ldpc_simulate_diag_rm run the host loop of ldpc_simulate / _diag with the profile on the channel and
 * the counters; the decode is untouched. */
typedef struct {
    const uint8_t *punctured_packed;  /* device, ceil(n/8) bytes, bit j at byte j/8 bit j%8 (as codeword_packed); NULL = none */
    const uint8_t *shortened_packed;  /* device, same format; NULL = none */
    const uint8_t *count_packed;      /* device, same format: bits that the error counters look at; NULL = all n bits */
    float short_llr;                  /* magnitude of a shortened bit's LLR; read only when shortened_packed != NULL */
} ldpc_rate_match;

int ldpc_channel_awgn_rm(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                         float scale, float shift, const uint8_t *codeword_packed, const ldpc_rate_match *rm, void *stream);
int ldpc_channel_awgn_mix_rm(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                             const float *scale_tab, const float *shift_tab, int32_t n_points,
                             const uint8_t *codeword_packed, const ldpc_rate_match *rm, void *stream);
int ldpc_sim_count_rm(int64_t *state, const uint8_t *packed_bits, const int32_t *iterations, int64_t batch, int32_t n,
                      const uint8_t *codeword_packed, int64_t max_frames, int64_t max_errors, const ldpc_rate_match *rm,
                      void *stream);
int ldpc_sim_count_diag_rm(int64_t *state, int64_t *diag, int32_t T, int64_t capture,
                           const uint8_t *packed_bits, const int32_t *iterations, const uint8_t *success,
                           int64_t batch, int32_t n, const uint8_t *codeword_packed, uint64_t block_first_frame,
                           int64_t max_frames, int64_t max_errors, void *scratch, size_t scratch_bytes,
                           const ldpc_rate_match *rm, void *stream);
int ldpc_simulate_rm(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_rate_match *rm, int64_t out_state[8],
                     void *workspace, size_t workspace_bytes, void *stream);
int ldpc_simulate_diag_rm(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_rate_match *rm, int64_t capture,
                          int64_t out_state[8], int64_t *out_diag /* host, ldpc_sim_diag_words(T of d, capture) */,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---- random codewords: a device encoder and a channel that reads one codeword per frame --------
 * With one codeword for every frame of a point -- all-zero by default -- a punctured bit that is never recovered keeps
 * posterior 0, decides 0 and counts as correct, and sign-asymmetric decoder rules are never exercised.  These entry points
 * draw a fresh codeword per frame from the counter-based stream.  Everything above is unchanged.
 *
 * Encoder.  A systematic encoder of a binary linear code in one format for sparse and dense codes (host arrays, copied to
 * the device of the calling thread):
 *     p_r = XOR of u_i over i in info_idx[row_ptr[r] .. row_ptr[r+1])   and, with accumulate != 0 and r > 0, XOR p_{r-1}
 *     c[info_pos[i]] = u_i  (i < k),   c[parity_pos[r]] = p_r  (r < n - k)
 * ldpc_encoder_create returns LDPC_ERR_ARG unless n >= 1, 0 <= k <= n, info_pos[k] and parity_pos[n-k] are together a
 * permutation of 0 .. n-1, row_ptr[n-k+1] starts at 0 and is monotone and every info_idx is in 0 .. k-1 (all checked before a
 * device is touched), and LDPC_ERR_UNSUPPORTED when a frame does not fit the kernel's LDS (n above roughly 130000).
 *
 * Rows are in the decoders' packed format -- bit j at byte j/8, bit j%8 -- and rows are packed: codewords_packed[batch]
 * [ceil(n/8)], info_packed[batch][ceil(k/8)] (device, any alignment; the stride is 250 bytes for n = 1998).  Bits at and
 * beyond n (k) in a row's last byte are written 0 (ignored on input).
 *
 * ldpc_encode : codewords of the given information rows.
 * ldpc_encode_random : codewords of frames first_frame .. first_frame + batch - 1 of the information-bit stream, and the
 *   information rows themselves when info_packed != NULL.  Information bit i of frame f is bit i % 32 of word x[(i / 32) % 4] of
 *     (x0, x1, x2, x3) = Philox4x32-10(counter = (f & 0xffffffff, f >> 32, 0x80000000 | (i / 128), stream_id),
 *                                      key = (seed & 0xffffffff, seed >> 32))
 *   -- the rounds of the noise stream above.  That stream's third counter word is a quad index below 2^29 + 256, so the set
 *   top bit keeps the two disjoint under one (seed, stream_id).  The codeword of frame f does not depend on the block it is
 *   drawn in.
 * Both: LDPC_ERR_ARG for batch < 0; then batch == 0 returns LDPC_OK without touching a pointer or a device; then LDPC_ERR_ARG
 * for a NULL encoder or a NULL row pointer (info_packed of ldpc_encode_random may be NULL).  Asynchronous on `stream`,
 * allocate nothing, safe under stream capture.
 *
 * ldpc_channel_awgn_cw : ldpc_channel_awgn_rm with the codeword bits of frame b read from row b of codewords_packed[batch]
 *   [ceil(n/8)] (rm == NULL: ldpc_channel_awgn).  Frame b equals the one-codeword call of that one frame with that row, bit
 *   for bit.  Argument checks as ldpc_channel_awgn_rm; codewords_packed must not be NULL when batch > 0.
 *
 * ldpc_simulate_enc : ldpc_simulate (capture < 0, out_diag unused) or ldpc_simulate_diag (capture >= 0), with rm as the _rm
 *   forms take it (NULL: none), on a fresh codeword per frame.  Per block: ldpc_encode_random with the point's seed, stream_id
 *   and frame indices, ldpc_channel_awgn_cw, ldpc_decode, the packed decisions XORed with the codeword rows, and the counters
 *   above against the all-zero word -- the code is linear, so popcount((d ^ c) & mask) is the error count and d satisfies H
 *   exactly when d ^ c does; `success` comes from the decoder.  Records, replay and the independence of block and poll_blocks
 *   are those of ldpc_simulate_diag; a recorded frame is drawn again by ldpc_encode_random(batch = 1, first_frame = record[0])
 *   and ldpc_channel_awgn_cw of that row.  desc->codeword_packed must be NULL, the encoder's n the decoder's and both on one
 *   device (LDPC_ERR_ARG); float64 decoders: LDPC_ERR_UNSUPPORTED.  workspace: ldpc_simulate_enc_workspace_bytes(d, block,
 *   capture) -- the plain workspace plus the block's codeword rows; the existing sizes do not change.  Synchronous, as
 *   ldpc_simulate. */
typedef struct ldpc_encoder ldpc_encoder;

int ldpc_encoder_create(ldpc_encoder **out, int32_t n, int32_t k, const int32_t *info_pos, const int32_t *parity_pos,
                        const int32_t *row_ptr, const int32_t *info_idx, int32_t accumulate);
void ldpc_encoder_destroy(ldpc_encoder *e);
int ldpc_encode(const ldpc_encoder *e, const uint8_t *info_packed, int64_t batch, uint8_t *codewords_packed, void *stream);
int ldpc_encode_random(const ldpc_encoder *e, int64_t batch, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                       uint8_t *codewords_packed, uint8_t *info_packed /* or NULL */, void *stream);
int ldpc_channel_awgn_cw(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                         float scale, float shift, const uint8_t *codewords_packed, const ldpc_rate_match *rm, void *stream);
size_t ldpc_simulate_enc_workspace_bytes(const ldpc_decoder *d, int64_t block, int64_t capture);
int ldpc_simulate_enc(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_encoder *e, const ldpc_rate_match *rm,
                      int64_t capture, int64_t out_state[8], int64_t *out_diag /* host, or NULL when capture < 0 */,
                      void *workspace, size_t workspace_bytes, void *stream);

/* ---- symbol channel: Gray-mapped QAM over AWGN or Rayleigh fading, max-log and exact demappers -
 * The channels above are binary-input AWGN.  The bit levels of a Gray-mapped 16- / 64- / 256-QAM symbol are unequal channels
 * and not output-symmetric, so they need the per-frame codewords of the section above.  Everything above is unchanged.
 *
 * Modulation.  m = bits_per_symbol in {1, 2, 4, 6, 8}: BPSK, QPSK, 16-, 64-, 256-QAM, every constellation of unit average
 * energy.  A frame of n bits is S = ceil(n / m) symbols.  Transmit index t = s * m + k is bit k of symbol s and carries the
 * codeword bit of variable position[t] (an interleaver: a permutation of 0 .. n-1 on the device, which the caller vouches for;
 * NULL is the identity).  Transmit indices >= n in the last symbol are pad bits: sent as 0, nothing is stored for them.
 * For m >= 2 the first h = m / 2 bits of a symbol label the I axis and the next h the Q axis; m = 1 has an I axis (h = 1) only.
 * An axis is Gray-labelled 2^h-PAM: level index i = gray_to_binary(b_0 .. b_{h-1}) with b_0 the most significant bit (the
 * running XOR), integer amplitude a = (2^h - 1) - 2 i.  So b_0 = 0 is the positive half and a lone bit 0 is +1: the decoders'
 * convention, bit 0 -> positive LLR.
 *
 * Noise stream.  Symbol s of frame f draws
 *     (x0, x1, x2, x3) = Philox4x32-10(counter = (f & 0xffffffff, f >> 32, 0x40000000 | s, stream_id),
 *                                      key = (seed & 0xffffffff, seed >> 32))
 * The BI-AWGN stream's third counter word is a quad index below 2^29 + 256 and the information-bit stream sets the top bit, so
 * the three are disjoint under one (seed, stream_id) as long as S < 2^29 (LDPC_ERR_UNSUPPORTED otherwise).
 *     (zI, zQ) = the Box-Muller pair of (x0, x1) exactly as the noise stream above forms z[4q], z[4q+1]; m = 1 uses zI only
 *     fading 0:  g = 1.0f (x2, x3 unused)
 *     fading 1:  g = sqrtf(-logf(u(x2))): Rayleigh amplitude with E g^2 = 1, independent per symbol, known to the receiver
 * A frame draws the same zI, zQ with and without fading.
 *
 * Received sample and demapper, all fp32, every multiply and add rounded on its own (no fused multiply-add).  `amp` is the
 * constellation's half-spacing over the per-dimension noise standard deviation.  Per axis, with sent amplitude a:
 *     e = g * amp;   v = e * (float)a + z
 *     for every candidate a':  t = v - e * (float)a',  D(a') = t * t
 *     bit k of the axis:       llr = 0.5f * (min_{a': b_k = 1} D - min_{a': b_k = 0} D)
 * the max-log LLR, exact for BPSK and QPSK; llr[b][position[t]] receives it.  With N0 = 10^(-snr_db / 10) and Es = 1:
 * BPSK has real noise of variance N0, amp = 1 / sqrt(N0); m >= 2 has N0 / 2 per dimension and half-spacing
 * d = sqrt(3 / (2 (4^h - 1))), amp = d / sqrt(N0 / 2).  2 amp is the `scale` of ldpc_channel_awgn for m = 1 and m = 2, and QPSK
 * at snr_db is, in law, the BI-AWGN channel at the same snr_db.
 *
 * ldpc_channel_sym : llr [batch][n] fp32 (device, 4-byte aligned) of frames first_frame .. first_frame + batch - 1.
 *   codeword_stride = ceil(n / 8): one packed row per frame, as ldpc_encode_random writes them; 0: one word for every frame;
 *   codewords_packed NULL: the all-zero word.  received, when not NULL: fp32 [batch][S][4] = (vI, vQ, e, 0.0f), 16-byte
 *   aligned, vQ = 0.0f for m = 1 -- the samples for a constellation plot or a demapper of the caller's own.
 *   LDPC_ERR_ARG for batch < 0, n < 1, a NULL mod, bits_per_symbol outside {1, 2, 4, 6, 8}, fading outside {0, 1}, amp not
 *   finite or < 0, a stride other than 0 and ceil(n / 8); LDPC_ERR_UNSUPPORTED for S >= 2^29; then batch == 0 returns LDPC_OK
 *   without touching a device pointer; then LDPC_ERR_ARG for a NULL or misaligned llr and a misaligned received.
 *   Asynchronous on `stream`, allocates nothing, safe under stream capture.
 *
 * ldpc_simulate_sym : the loop of ldpc_simulate_enc with this channel.  Per block: ldpc_encode_random when e != NULL,
 *   otherwise desc->codeword_packed (NULL: all-zero) for every frame; ldpc_channel_sym; ldpc_decode; the decisions XORed with
 *   the codeword rows (e == NULL: the counters compare with the one word instead); the counters.  capture < 0: no diagnostics
 *   (out_diag unused).  Records, replay and the independence of block and poll_blocks are those of ldpc_simulate_enc; a
 *   recorded frame is drawn again by ldpc_encode_random and ldpc_channel_sym with batch = 1, first_frame = record[0].
 *   desc->scale and desc->shift are ignored; desc->codeword_packed must be NULL when e != NULL.  float64 decoders:
 *   LDPC_ERR_UNSUPPORTED.  workspace: ldpc_simulate_sym_workspace_bytes(d, block, capture).  Synchronous, as ldpc_simulate.
 *
 * ldpc_channel_sym_mix : ldpc_channel_sym with the SNR point a function of the frame, for training: frame
 *   f = first_frame + b is drawn at amp = amp_tab[f mod n_points] (amp_tab: fp32 [n_points] on the device, 4-byte aligned,
 *   1 <= n_points <= 4096, its entries the caller's responsibility; batch <= 2^31 - 1; mod->amp is ignored) and receives, bit
 *   for bit, what ldpc_channel_sym gives it at that amp, whatever block it is drawn in: every run of n_points consecutive
 *   frames holds each point once, as under ldpc_channel_awgn_mix.  Codeword arguments as in ldpc_channel_sym.  targets, when
 *   not NULL: fp32 [batch][n] (device, 4-byte aligned), targets[b][j] = 0.0f / 1.0f, the codeword bit of variable j that frame
 *   b sent (all +0.0f for the all-zero word) -- the `targets` of the ldpc_train_joint* entry points, written by the lane that
 *   sends the bit.  Nothing is stored for pad bits in either output.
 *   LDPC_ERR_ARG for batch < 0, n < 1, a NULL mod, bits_per_symbol outside {1, 2, 4, 6, 8}, fading outside {0, 1}, a stride
 *   other than 0 and ceil(n / 8), n_points outside 1 .. 4096, batch > 2^31 - 1, first_frame + batch beyond 2^64, a NULL
 *   amp_tab with batch > 0; LDPC_ERR_UNSUPPORTED for S >= 2^29; then batch == 0 returns LDPC_OK without touching a device
 *   pointer; then LDPC_ERR_ARG for a NULL or misaligned llr, a misaligned targets and a misaligned amp_tab.
 *   Asynchronous on `stream`, allocates nothing, safe under stream capture.
 *
 * Demappers.  With L = 2^h candidate amplitudes a' per axis, D(a') as above and m_b = min_{a': b_k = b} D(a'), all fp32 and
 * every operation rounded on its own:
 *     LDPC_DEMAP_MAXLOG:  llr_k = 0.5f * (m1 - m0), the rule above -- what the entry points without a demapper argument use
 *     LDPC_DEMAP_EXACT:   S_b = sum_{a': b_k = b} expf(-0.5f * (D(a') - m_b)), summed in ascending level index
 *                         c_k = logf(S_0) - logf(S_1);   llr_k = 0.5f * (m1 - m0) + c_k
 * the exact log-MAP LLR of the axis (the log-sum-exp rule).  Each set is normalised by its own minimum, so 1 <= S_b <= L / 2,
 * |c_k| <= log(L / 2), and the exact LLR is the max-log LLR plus a bounded correction: finite wherever the max-log LLR is.
 * (A form normalised once by the global minimum underflows: the far set's sum rounds to 0 and its logf to -inf.)  For h = 1
 * (BPSK, QPSK) each set has one element, S_b = 1.0f, c_k = +0.0f and the exact rule is the max-log rule bit for bit.  With
 * e = 0 every D is equal and the LLR is +0.0f, an erasure, under both.  expf and logf are the device library's (1 ulp).
 *
 * ldpc_demap_sym : LLRs from received samples.  received: fp32 [batch][S][4] = (vI, vQ, e, 0) on the device, 16-byte aligned,
 *   the layout ldpc_channel_sym writes (vQ and the fourth word are not read for m = 1 / at all).  llr [batch][n] fp32 (device,
 *   4-byte aligned) receives, at variable position[t], the LLR of transmit bit t under `demapper`; nothing is stored for pad
 *   bits.  mod->amp and mod->fading are ignored (e travels with the samples); mod->position is honoured.  With
 *   LDPC_DEMAP_MAXLOG the samples ldpc_channel_sym wrote give the LLRs it wrote, bit for bit; with LDPC_DEMAP_EXACT those
 *   ldpc_channel_sym_dm wrote.
 *   LDPC_ERR_ARG for batch < 0, n < 1, a NULL mod, bits_per_symbol outside {1, 2, 4, 6, 8}; LDPC_ERR_UNSUPPORTED for
 *   S >= 2^29; LDPC_ERR_ARG for a demapper outside {0, 1}; then batch == 0 returns LDPC_OK without touching a device pointer;
 *   then LDPC_ERR_ARG for a NULL or misaligned llr and a NULL or misaligned received.
 *   Asynchronous on `stream`, allocates nothing, safe under stream capture.
 *
 * ldpc_channel_sym_dm, ldpc_channel_sym_mix_dm, ldpc_simulate_sym_dm : ldpc_channel_sym, ldpc_channel_sym_mix and
 *   ldpc_simulate_sym with the demapper chosen (LDPC_ERR_ARG outside {0, 1}, checked after the modulation); the three entry
 *   points without the argument are these with LDPC_DEMAP_MAXLOG.  Noise, fading, received samples, targets and workspace
 *   sizes do not depend on the demapper.
 *
 * Not provided: rate matching together with a modulation, block fading, a training step that fuses this draw into the
 * decode, fp64 LLRs, a table-driven or globally normalised fast form of the exact rule, demapping with decoder feedback.
 * (PSK above 4 points, APSK and every other labelled point set: the constellation channel below.) */
enum { LDPC_DEMAP_MAXLOG = 0, LDPC_DEMAP_EXACT = 1 };

typedef struct {
    int32_t bits_per_symbol;      /* 1, 2, 4, 6, 8 */
    int32_t fading;               /* 0 none, 1 Rayleigh per symbol */
    float   amp;                  /* finite, >= 0 */
    const int32_t *position;      /* device, n entries, or NULL */
} ldpc_modulation;

int ldpc_channel_sym(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                     const ldpc_modulation *mod, const uint8_t *codewords_packed, int64_t codeword_stride,
                     void *received /* or NULL */, void *stream);
int ldpc_channel_sym_mix(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                         const ldpc_modulation *mod, const float *amp_tab, int32_t n_points,
                         const uint8_t *codewords_packed, int64_t codeword_stride,
                         void *targets /* or NULL */, void *stream);
size_t ldpc_simulate_sym_workspace_bytes(const ldpc_decoder *d, int64_t block, int64_t capture);
int ldpc_simulate_sym(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_encoder *e /* or NULL */,
                      const ldpc_modulation *mod, int64_t capture, int64_t out_state[8], int64_t *out_diag,
                      void *workspace, size_t workspace_bytes, void *stream);
int ldpc_demap_sym(void *llr, int64_t batch, int32_t n, const ldpc_modulation *mod, int32_t demapper,
                   const void *received, void *stream);
int ldpc_channel_sym_dm(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                        const ldpc_modulation *mod, const uint8_t *codewords_packed, int64_t codeword_stride,
                        void *received /* or NULL */, int32_t demapper, void *stream);
int ldpc_channel_sym_mix_dm(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                            const ldpc_modulation *mod, const float *amp_tab, int32_t n_points,
                            const uint8_t *codewords_packed, int64_t codeword_stride,
                            void *targets /* or NULL */, int32_t demapper, void *stream);
int ldpc_simulate_sym_dm(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_encoder *e /* or NULL */,
                         const ldpc_modulation *mod, int32_t demapper, int64_t capture, int64_t out_state[8],
                         int64_t *out_diag, void *workspace, size_t workspace_bytes, void *stream);

/* ---- constellation channel: a table of up to 64 labelled points, demapped jointly over all points ----
 * The symbol channel above rests on a Gray-labelled square grid that separates into two PAM axes.  This one takes the
 * constellation as a table: 8-PSK, APSK, any labelling, rotated, shaped or learned point sets.  Everything above is unchanged.
 *
 * Constellation.  m = bits_per_symbol in 1 .. 6, `points` an fp32 table [2^m][2] = (xI, xQ) on the device, 8-byte aligned,
 * whose contents the caller vouches for (finite; unit mean energy if `amp` is to mean what it means below).  The frame layout
 * is the symbol channel's: S = ceil(n / m) symbols, transmit index t = s * m + k is bit k of symbol s and carries the codeword
 * bit of variable position[t] (NULL: the identity), pad bits are sent as 0 and never stored.  The symbol's label is
 * l = sum_k b_k 2^k (bit k of the symbol at bit k) and the sent point is points[l]: the labelling is the order of the table,
 * nothing else.
 *
 * Noise stream: the symbol channel's, word for word -- Philox4x32-10 with counter (f lo, f hi, 0x40000000 | s, stream_id),
 * (zI, zQ) the Box-Muller pair of (x0, x1), g = 1.0f or sqrtf(-logf(u(x2))) under fading, S < 2^29.  A table that holds a QAM
 * grid sees the noise and fading that ldpc_channel_sym gives that scheme at the same (seed, stream_id, frame).  The noise is
 * complex for every m, m = 1 included.
 *
 * Received sample and distances, all fp32, every multiply and add rounded on its own (no fused multiply-add):
 *     e  = g * amp
 *     vI = (e * xI_l) + zI;   vQ = (e * xQ_l) + zQ
 *     for every candidate c = 0 .. 2^m - 1:  tI = vI - (e * xI_c);  tQ = vQ - (e * xQ_c);  D_c = (tI * tI) + (tQ * tQ)
 *     m_b(k) = min over c with bit k of c equal to b of D_c
 *     LDPC_DEMAP_MAXLOG:  llr_k = 0.5f * (m_1 - m_0)
 *     LDPC_DEMAP_EXACT:   S_b = sum_{c: bit k of c = b} expf(-0.5f * (D_c - m_b)), summed in ascending c
 *                         llr_k = 0.5f * (m_1 - m_0) + (logf(S_0) - logf(S_1))
 * the normalisation and summation order of the exact rule above: 1 <= S_b <= 2^(m-1), so |correction| <= (m - 1) log 2.  For
 * m = 1 the exact rule is the max-log rule bit for bit; e = 0 gives +0.0f under both.  `amp` is 1 / sigma, sigma = sqrt(N0 / 2)
 * the per-dimension noise standard deviation: with Es = 1, amp = sqrt(2 * 10^(snr_db / 10)), for every m.
 *
 * ldpc_channel_con : ldpc_channel_sym_dm on the table.  llr, codewords_packed, codeword_stride, received ([batch][S][4] =
 *   (vI, vQ, e, 0.0f), or NULL) and demapper as there.
 *   LDPC_ERR_ARG for batch < 0, n < 1, a NULL con, bits_per_symbol outside 1 .. 6, a NULL points, fading outside {0, 1}, amp
 *   not finite or < 0, a stride other than 0 and ceil(n / 8), a demapper outside {0, 1}; LDPC_ERR_UNSUPPORTED for S >= 2^29;
 *   then batch == 0 returns LDPC_OK without touching a device pointer; then LDPC_ERR_ARG for a NULL or misaligned llr, a
 *   misaligned received and a points that is not 8-byte aligned.
 * ldpc_channel_con_mix : ldpc_channel_sym_mix_dm on the table: amp = amp_tab[f mod n_points] (con->amp is ignored), targets as
 *   there; a frame receives, bit for bit, what ldpc_channel_con gives it at that amp.  Checks as ldpc_channel_con, with, after
 *   the demapper: n_points outside 1 .. 4096, batch > 2^31 - 1, first_frame + batch beyond 2^64, a NULL amp_tab with
 *   batch > 0; and a misaligned targets and amp_tab among the pointers.
 * ldpc_demap_con : ldpc_demap_sym on the table.  con->amp and con->fading are ignored, con->position is honoured.  The samples
 *   ldpc_channel_con wrote give, under the same demapper, the LLRs it wrote, bit for bit.  Checks: batch, n, con,
 *   bits_per_symbol, points, demapper, S, batch == 0, then llr, received (NULL or not 16-byte aligned) and points.
 * ldpc_simulate_con : the loop of ldpc_simulate_sym_dm with ldpc_channel_con as the channel; records, replay, workspace
 *   (ldpc_simulate_sym_workspace_bytes) and everything else as there.
 * The three channel entry points are asynchronous on `stream`, allocate nothing and are safe under stream capture.
 *
 * ldpc_demap_con_prior : ldpc_demap_con given a priori LLRs of the frame's variables, returning *extrinsic* LLRs -- the
 *   demapper of iterative demapping with decoder feedback (BICM-ID).  Frame layout, labels, received = (vI, vQ, e, 0), the
 *   distances D_c and the candidate order are ldpc_demap_con's; positive means bit 0.  `prior` and `prior_sub` are fp32
 *   [batch][n] on the device in variable order.  For the symbol's bits k = 0 .. m-1, bit k carrying variable j_k, all fp32,
 *   every operation rounded on its own (no fused multiply-add):
 *     La_k  = prior_scale * (prior[j_k] - prior_sub[j_k])     (prior_sub == NULL: prior_scale * prior[j_k]);
 *             +0.0f for the bits past n in the last symbol
 *     A_c   = the sum over the set bits j of c, in ascending j and starting from 0.0f, of La_j
 *             (= A_{c without its highest set bit} + La_{that bit}: the same roundings)
 *     Lam_c = D_c + (2.0f * A_c)
 *     M_b(k) = min over c with bit k of c equal to b of Lam_c
 *     LDPC_DEMAP_MAXLOG:  llr_k = 0.5f * (M_1 - M_0) - La_k
 *     LDPC_DEMAP_EXACT:   S_b = sum_{c: bit k of c = b, ascending c} expf(-0.5f * (Lam_c - M_b))
 *                         llr_k = (0.5f * (M_1 - M_0) + (logf(S_0) - logf(S_1))) - La_k
 *   The bit's own prior is subtracted at the end: the output is what the channel and the *other* bits of the symbol say about
 *   bit k.  With every La +0.0f or -0.0f, Lam_c == D_c exactly and the result is ldpc_demap_con's under both rules, bit for
 *   bit but for the sign of a zero: where ldpc_demap_con gives -0.0f (0.5f times a negative difference of the smallest
 *   subnormal, which rounds to -0.0f) and the bit's prior is -0.0f, the final subtraction gives +0.0f.  With
 *   prior == NULL the call *is* ldpc_demap_con (its kernel is launched; prior_scale is still checked).  For m = 1 the exact
 *   rule is the max-log rule.  The priors must be finite: +-inf and NaN are outside the contract (inf - inf in Lam_c).
 *   The decoder's extrinsic is its posterior minus what it was given: prior = the posterior, prior_sub = the LLRs it decoded.
 *   Aliasing: llr may be `prior` or `prior_sub` itself (the same pointer, not an overlapping range).  A lane reads the priors
 *   of its own symbol's variables, all before it stores, and stores to those variables only; that is safe as long as
 *   `position` is a permutation of 0 .. n-1, which the caller vouches for as everywhere above.
 *   Checks, in ldpc_demap_con's order: batch, n, con, bits_per_symbol, points, demapper, then a prior_scale that is not
 *   finite, S, batch == 0, then llr, received (NULL or not 16-byte aligned), a prior that is not 4-byte aligned, a prior_sub
 *   that is not 4-byte aligned, a prior_sub without a prior, and points.  Asynchronous on `stream`, allocates nothing, safe
 *   under stream capture.
 *
 * Not provided: more than 64 points, fp64, a reduced-search or table-driven fast form of the joint rule, a prior form of the
 * separable Gray demapper (ldpc_demap_sym: Gray labels gain nothing from feedback), decoder messages carried across
 * demapping rounds, rate matching with a constellation, block fading, the standards' own APSK bit maps (pass the standard's
 * table). */
typedef struct {
    int32_t bits_per_symbol;      /* m, 1 .. 6 */
    int32_t fading;               /* 0 none, 1 Rayleigh per symbol */
    float   amp;                  /* finite, >= 0 */
    const int32_t *position;      /* device, n entries, or NULL */
    const float   *points;        /* device fp32 [2^m][2] = (xI, xQ), 8-byte aligned; the caller vouches for its contents */
} ldpc_constellation;

int ldpc_channel_con(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                     const ldpc_constellation *con, const uint8_t *codewords_packed, int64_t codeword_stride,
                     void *received /* or NULL */, int32_t demapper, void *stream);
int ldpc_channel_con_mix(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                         const ldpc_constellation *con, const float *amp_tab, int32_t n_points,
                         const uint8_t *codewords_packed, int64_t codeword_stride,
                         void *targets /* or NULL */, int32_t demapper, void *stream);
int ldpc_demap_con(void *llr, int64_t batch, int32_t n, const ldpc_constellation *con, int32_t demapper,
                   const void *received, void *stream);
int ldpc_demap_con_prior(void *llr, int64_t batch, int32_t n, const ldpc_constellation *con, int32_t demapper,
                         const void *received, const void *prior /* fp32 [batch][n], or NULL */,
                         const void *prior_sub /* fp32 [batch][n], or NULL */, float prior_scale, void *stream);
int ldpc_simulate_con(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_encoder *e /* or NULL */,
                      const ldpc_constellation *con, int32_t demapper, int64_t capture, int64_t out_state[8],
                      int64_t *out_diag, void *workspace, size_t workspace_bytes, void *stream);

const char *ldpc_last_error(void);
int ldpc_abi_version(void);
/* sha256 (hex) over the sources and the compile recipe this library was built from, embedded at build time
 * (-DLDPC_SRC_HASH=...; "unknown" for a hand build).  The Python loader compares it with the sources on disk and
 * refuses a library that does not match -- file times say nothing after a copy to another machine. */
const char *ldpc_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_HIP_H */
