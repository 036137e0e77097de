/*
 * ldpc_hip_debug.h -- measurement and test hooks of libldpc_hip.so.
 *
 * NOT part of the product ABI (include/ldpc_hip.h): nothing here is needed to decode, and no
 * reference interface corresponds to it.  bench.py uses ldpc_debug_sweep to time one sweep kernel
 * with HIP events; the parity tests use the two state dumps to compare per-edge check-to-variable
 * messages (for RCQ: the 3-bit quantiser codes the reference emits, rcq_decoder.py:244-246) on BOTH
 * engines; ldpc_debug_resident_kernel lets a test assert WHICH resident kernel and table flags a decode runs,
 * ldpc_debug_boundary_kernels which layout kernels a streaming decode takes for given caller pointers,
 * ldpc_debug_launch_geometry which syndrome kernel and which cn_gather tile mapping a batch's tile count selects.
 */
#ifndef LDPC_HIP_DEBUG_H
#define LDPC_HIP_DEBUG_H

#include "ldpc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Run ONE sweep of iteration `iter` on the state left in `workspace` by a previous
 * ldpc_decode (streaming engine) of the same batch: which = 0 check-node (CN->VN) sweep,
 * 1 variable-node sweep. */
int ldpc_debug_sweep(const ldpc_decoder *d, int64_t batch, int32_t which, int32_t iter,
                     void *workspace, size_t workspace_bytes, void *stream);

/* Byte offsets of the streaming engine's state arrays inside a workspace for `batch`
 * codewords: out8 = { VEC, tiles, llrT, v2c, c2v, postT, bitsT, done }.  Messages are laid out
 * [tile][edge][W] with W = 64*VEC codewords innermost.  c2v is where the last executed iteration
 * left its messages in a decode capped at max_iterations (ldpc_decode_capped; <= 0: ldpc_decode). */
int ldpc_debug_workspace_layout(const ldpc_decoder *d, int64_t batch, int32_t max_iterations, int64_t out8[8]);

/* LDS-resident engine: decode llr[batch][n] (posterior[batch][n] and iterations[batch] out, as
 * ldpc_decode) and ALSO copy every codeword's check-to-variable messages of its last executed
 * iteration out of LDS into c2v_out[batch][E] (decoder dtype, CSR edge order; RCQ decoders hold the
 * reconstructed values (1 - 2*sign) * tau[level], from which the test recovers the codes).
 * max_iterations > 0 runs at most that many of the decoder's iterations, as ldpc_decode_capped;
 * max_iterations <= 0 runs the decoder's T. */
int ldpc_debug_resident_c2v(const ldpc_decoder *d, const void *llr, int64_t batch, int32_t early_stop,
                            int32_t max_iterations, void *posterior, int32_t *iterations, void *c2v_out,
                            void *stream);

/* The kernel a decode of d runs on the LDS-resident engine (host only, no device is touched), for early_stop != 0 or the
 * fixed-T decode: out12 = { plan, G, FORM, BPC, NL, MS, row stride, SPLIT, unit_alpha, rcq_zero0, oms_alpha, alpha_in_lds }.
 * plan: 0 general (streaming variable loop), 1 register-held variable state, 2 the compact fixed-T plan.  G, FORM
 * (LDPC_C2V_*), BPC (one beta slot per check), NL (compile-time level count, 0: run time), MS (compile-time row stride, 0:
 * run time) and SPLIT are the template arguments of resident_decode; row stride is the plan's own.  The last four are the
 * table properties the kernel branches on: every alpha exactly 1, every quantiser's tau_0 == 0, a check-side alpha table
 * of the offset form, the alpha table staged in LDS.  The launcher and this hook read one selection (csrc/ldpc_hip.hip,
 * resident_kernel).  G is the kernel's (1 for fp64: one codeword in the slots of a float pair).  LDPC_ERR_UNSUPPORTED when the
 * decoder's mode does not put it on the resident engine or its schedule is layered (those never launch resident_decode). */
int ldpc_debug_resident_kernel(const ldpc_decoder *d, int32_t early_stop, int32_t out12[12]);

/* The kernels that move a streaming decode's rows between the caller's layout and the tiles (host only, no device is
 * touched; llr, posterior and bits are compared, never dereferenced, and may be NULL as in ldpc_decode).  For a decode of
 * `batch` codewords running at most max_iterations of the decoder's iterations (<= 0: its T), through ldpc_decode /
 * ldpc_decode_capped or (saving != 0) ldpc_decode_saving: out5 = { VEC, input bytes, fused entrance, output path, output
 * bytes }.  VEC: codewords per lane of a tile (64 * VEC codewords wide).  Input bytes: what one lane moves per access on the
 * caller's side of the entrance pass, 16 / 8 / 4 (transpose_in_v), 0 the scalar transpose_in.  Fused entrance: 1 when the
 * code-pair form's transpose_in_q4 runs instead (16-byte rows only).  Output path: 0 none (neither bits nor posterior), 1
 * the layout pass (transpose_out_v, or the scalar transpose_out when output bytes is 0), 2 the last variable pass stores the
 * caller's rows itself (vn_last_rows, output bytes / 4 floats per store).  The launcher and this hook read one selection
 * (csrc/ldpc_hip.hip, boundary_kernels).  LDPC_ERR_UNSUPPORTED when the decode runs an LDS-resident kernel (those read and
 * write the caller's rows element by element) or, with saving != 0, the decoder has no gradient path. */
int ldpc_debug_boundary_kernels(const ldpc_decoder *d, int64_t batch, int32_t max_iterations, int32_t saving,
                                const void *llr, const void *posterior, const int32_t *bits, int32_t out5[5]);

/* The launch rules of a streaming decode that depend on how many tiles the batch is cut into (host only, no device is
 * touched): out8 = { VEC, tiles, syndrome chunks, gather XCD tiles, gather padded tiles, 0, 0, 0 }.  VEC and tiles as
 * ldpc_debug_workspace_layout.  Syndrome chunks: the blocks per tile of the syndrome + latch pass; 2 or more is
 * syndrome_latch_chunks (per-tile ticket and OR word in the workspace, both zero between launches), 1 the one-block
 * syndrome_latch, 0 a layered schedule (its kernels check the syndrome themselves).  Gather XCD tiles: the tile count
 * handed to cn_gather when it runs the XCD-affine tile mapping (workgroup b works on tile 8 * (b / 8 / check blocks) + b % 8),
 * 0 for the tile-major mapping or a decoder that does not launch cn_gather (any form but the fused RCQ iteration);
 * gather padded tiles: the tiles its grid covers -- under the XCD mapping the next multiple of 8, whose surplus workgroups
 * exit at once -- else `tiles`.  The last three words are spare and zero.  The launchers and this hook read one pair of
 * functions (csrc/ldpc_hip.hip, syndrome_chunks and gather_tiles).  LDPC_ERR_UNSUPPORTED when the decode runs an
 * LDS-resident kernel: those have no tiles. */
int ldpc_debug_launch_geometry(const ldpc_decoder *d, int64_t batch, int64_t out8[8]);

/* Compact fixed-T plan of the LDS-resident engine (host only, no device is touched).  The kernel runs the variable at
 * position q = r*512 + w*64 + lane in round r (< 4) of wave w (< 8); cells[w*4 + r] describes cell (w, r): 0 empty,
 * 1..8 the one degree of all 64 lanes, 0x40 | degree one degree with some lanes empty, 0xff mixed (or degree 0).
 * d != NULL: the plan decoder d builds for its fixed-T decodes (the graph arguments are ignored; LDPC_ERR_UNSUPPORTED
 * when it has none).  d == NULL: the plan of the graph (n, m, E, check_ptr, var_idx as ldpc_graph_create), whether or
 * not a decoder's tables would let it take the compact geometry.  pos_of_var[n] receives every variable's position;
 * stats = { positions in use (highest + 1), largest per-wave cost, summed per-wave cost, mixed cells } under the body-cost
 * model of the variable phase (csrc/ldpc_hip.hip, cpt_body_cost).  Output pointers may be NULL. */
int ldpc_debug_compact_layout(const ldpc_decoder *d, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr,
                              const int32_t *var_idx, int32_t *pos_of_var, uint8_t cells[32], int32_t stats[4]);

/* Check table of the compact fixed-T plan (host only, arguments as ldpc_debug_compact_layout).  Checks are sorted by
 * descending degree and wave w runs positions 64w .. 64w+63; words[w] = d_lo | (d_hi - d_lo) << 8 | lanes << 16 with d_lo /
 * d_hi the smallest / largest degree among the wave's checks and `lanes` how many it holds (0: the whole word is 0).
 * Bit 31 marks a wave that runs the per-lane form of the check phase; every other wave runs d_lo edges on a scalar trip
 * count and only the d_hi - d_lo remaining ones under a lane mask.  d == NULL: the graph's table, bit 31 where d_lo < 4.
 * d != NULL: the table the decoder runs with -- every wave marked unless its check phase is the one-beta-per-check
 * select form (normalised min-sum or RCQ with tau_0 == 0, one beta slot per check). */
int ldpc_debug_compact_checks(const ldpc_decoder *d, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr,
                              const int32_t *var_idx, uint32_t words[8]);

/* Slot placement of the compact fixed-T plan and its LDS bank model (host only, arguments as ldpc_debug_compact_layout).
 * Check position p (< m) runs one check; its dc edges sit in the slots row * geometry[0] + p, rows 0 .. dc-1 in an order
 * the planner chooses.  slot_of_edge[E] (CSR edge order) and pos_of_check[m] describe the placement the plan ships;
 * model = { gather cost, gather groups, scatter cost, scatter groups } of one variable phase in LDS-array cycles: a group
 * is the 32 lanes of one ds_read_b64 (16 of one ds_write_b64) that hold at least one edge, its cost the largest number of
 * its lanes on one bank, slot mod 32 (slot mod 16).  base_* is the same for the placement the planner starts from: checks
 * in stable degree order, rows in CSR order, variables placed by the variables-only search.  geometry = { row stride,
 * slots Sc }.  Output pointers may be NULL. */
int ldpc_debug_compact_banks(const ldpc_decoder *d, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr,
                             const int32_t *var_idx, int32_t *slot_of_edge, int32_t *pos_of_check, int32_t model[4],
                             int32_t *base_slot_of_edge, int32_t *base_pos_of_check, int32_t base_model[4],
                             int32_t geometry[2]);

/* The variable sweep of the RCQ code-pair form turns every outgoing value v into the key
 * [m > 0] + [m >= t1] + [m >= t2] + [m >= t3] of m = |beta * v| (thresholds4[0] is not used; device pointers, thresholds
 * within [2^-50, 2^50]).  Runs BOTH device forms of that key on `count` arbitrary values: the float form the 4-level
 * kernels use (clamped differences, csrc/ldpc_kernels.hip key_pair4) and the integer compare chain it replaced. */
int ldpc_debug_key4(const float *values, int64_t count, float beta, const float thresholds4[4], uint8_t *keys_float,
                    uint8_t *keys_compare, void *stream);

/* Pass 1 of the resident check phase keeps the two smallest magnitudes m1 <= m2 and the xor of the bit patterns of a
 * check's inputs.  Runs BOTH device forms of it on values[rows][d] (device pointers, 1 <= d <= 32, row-major fp32, no
 * NaN): the one-value chain, and the edges in pairs (min3 / med3 / min and a three-input xor, csrc/ldpc_resident.hip
 * res_absorb2) with an odd last one through the one-value step.  m12_*[rows][2] receive { m1, m2 }, par_*[rows] the xor
 * word (bit 31 is the sign parity).  No degree-1 rule is applied: d == 1 leaves m2 = +inf. */
int ldpc_debug_min2(const float *values, int64_t rows, int32_t d, float *m12_chain, uint32_t *par_chain, float *m12_pair,
                    uint32_t *par_pair, void *stream);

/* The raw Philox4x32-10 words behind ldpc_channel_awgn (include/ldpc_hip.h): out4[count][4] (device) receives, for quad
 * i < count, the four words of counter (f & 0xffffffff, f >> 32, i % quads_per_frame, stream_id) with
 * f = first_frame + i / quads_per_frame, under key (seed & 0xffffffff, seed >> 32). */
int ldpc_debug_philox(uint32_t *out4, int64_t count, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                      int32_t quads_per_frame, void *stream);

/* The block-parallel layered decode's planner (csrc/ldpc_layer_plan.h) on a bare graph and layer partition; host only, no
 * device is touched.  kind 0: the min-sum forms (check records), 1: RCQ (code bytes).  LDPC_ERR_ARG for an invalid CSR or
 * partition.  out8 = { qualifies, codewords per workgroup, lanes per codeword, threads per workgroup, LDS bytes per
 * workgroup, dwords of a codeword's row, plan entries, mask words per check record } -- the geometry ldpc_decoder_info
 * reports under LDPC_MODE_BLOCK; all but the first 0 when the code does not qualify (ldpc_last_error says why). */
int ldpc_debug_layer_plan(int32_t n, int32_t m, int32_t n_edges, const int32_t *check_ptr, const int32_t *var_idx,
                          int32_t n_layers, const int32_t *layer_ptr, int32_t kind, int64_t out8[8]);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_HIP_DEBUG_H */
