// ldpc_layered_block.hip -- block-parallel layered decode (gfx950): lanes run over the CHECKS of one layer.
//
// LDPC_SCHED_LAYERED on a graph that declares layers (ldpc_graph_create_layered): a layer is a run of consecutive checks
// whose variable sets are pairwise disjoint, so its checks read and write disjoint posteriors and may be updated all at
// once.  Every step of the layered update is a single rounded operation (u = P - R, min1 / min2 with "first minimum is the
// arg-min", one product, one add; __fmul_rn / __fadd_rn close the only contraction hazard), so the result equals, bit for
// bit, the sequential walk over the same graph: layered_minsum_lds / layered_paper_lds (ldpc_layered.hip), which put
// their lanes on the edges of ONE check and run a dependent chain of m steps per iteration, and the streaming kernels
// layered_minsum / layered_rcq<VEC, true> (ldpc_kernels.hip).  Here the chain is the number of layers.
//
// A workgroup holds G codewords in LDS (layout and planner: ldpc_layer_plan.h).  Thread tid = g * lpc + j owns check j
// of the current layer for codeword g (j fastest: inside a codeword the lanes of a wave gather consecutive entries of
// the plan, and on a circulant consecutive posteriors apart from the wrap); a layer wider than lpc is walked in chunks
// j, j + lpc, ... with no barrier between them -- the checks are disjoint.  A thread makes two passes over its check's
// edges: (1) u = P - R, running min1 / min2 / sign parity; (2) u again, the new message r, P = u + r and the new record
// or code.  No array is sized by the degree.
//
// Previous messages: the min-sum forms keep the check record of layered_minsum_lds (m1, m2, one sign bit and one
// arg-min bit per edge) and recompute R from it with beta_{t-1} (a_{t-1}) of the plan entry -- the same operands through
// the same single operation give the bits a stored value would have; RCQ keeps the one-byte code per edge
// (level | sign << 7) of layered_paper_lds.
//
// Barriers: one per layer, two per iteration's syndrome under early stop.  EVERY lane of the workgroup reaches every
// barrier: the iteration loop runs until the workgroup's last live codeword has stopped (one LDS word read by all lanes
// after a barrier, so the exit is uniform), and a frozen or padding codeword's lanes skip the work of a layer, never
// its barrier.  No barrier stands under a per-codeword or per-lane condition.
#pragma once

#include "ldpc_kernels.hip"
#include "ldpc_layer_plan.h"

namespace ldpc {

struct BlockPlan {
    int n, m, L, W;                // W: 32-bit mask words of a check record (min-sum forms)
    int G, lpc;                    // codewords per workgroup, lanes per codeword
    unsigned row_words, rec_off;   // dwords of a codeword's LDS row (odd); where its records / codes start
    int entries;
    const int *layer_ptr;          // [L + 1]
    const int *entry_base;         // [L + 1]
    const int *deg;                // [m]
    const uint32_t *off;           // [entries] byte offset of the entry's posterior inside the row
    const float *beta_lay;         // [T][entries] beta_t of the entry's edge (lay_beta_gather), NULL: none
    const float *oms_lay;          // [T][entries] the offset form's check-side alpha, NULL: none
};

// FORM_NMS / FORM_OMS (AUX: a check-side alpha table exists) / FORM_RCQ (AUX: weighted, some beta != 1); ES: early stop
template <int FORM, bool ES, bool AUX>
__global__ __launch_bounds__(kBlkMaxThreads) void layered_block_lds(BlockPlan pl, const float *__restrict__ llr, long long batch,
                                                                    const float *__restrict__ thresholds, int n_levels,
                                                                    const int *__restrict__ q_of_iter, int T,
                                                                    int *__restrict__ bits, float *__restrict__ posterior,
                                                                    int *__restrict__ iterations, uint8_t *__restrict__ success,
                                                                    uint8_t *__restrict__ packed)
{
    static_assert(FORM == FORM_NMS || FORM == FORM_OMS || FORM == FORM_RCQ, "forms of the layered schedule");
    extern __shared__ __align__(16) float blk_smem[];
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & (kWave - 1);
    const int n = pl.n, m = pl.m, G = pl.G, lpc = pl.lpc, W = pl.W;
    const unsigned row_words = pl.row_words;
    const long long b0 = (long long)blockIdx.x * G;
    const int g = tid / lpc, j = tid - g * lpc;
    const bool mine = g < G && b0 + g < batch;                  // this lane's codeword exists
    int *flags = (int *)(blk_smem + (size_t)G * row_words);     // unsat[G], frozen[G], iters[G], live
    int *f_unsat = flags, *f_frozen = flags + G, *f_iters = flags + 2 * G, *f_live = flags + 3 * G;
    float *P = blk_smem + (size_t)(g < G ? g : 0) * row_words;  // this lane's row (lanes beyond G never touch it)
    unsigned *Rw = (unsigned *)(P + pl.rec_off);                // min-sum: m1[m] m2[m] sign[W][m] arg[W][m]
    uint8_t *Cd = (uint8_t *)(P + pl.rec_off);                  // RCQ: code of plan entry e at byte e

    // LLRs (coalesced, all lanes over one row at a time); records / codes: none (+0)
    for (int r = 0; r < G; ++r) {
        const bool have = b0 + r < batch;
        const float *src = llr + (size_t)(have ? b0 + r : 0) * n;
        float *row = blk_smem + (size_t)r * row_words;
        for (int x = tid; x < n; x += NT) row[x] = have ? __builtin_nontemporal_load(src + x) : 1.0f;
        for (unsigned x = (unsigned)n + tid; x < row_words; x += NT) row[x] = 0.0f;
    }
    if (tid < G) {
        f_unsat[tid] = 0;
        f_frozen[tid] = b0 + tid < batch ? 0 : 1;
        f_iters[tid] = T;
    }
    if (tid == 0) *f_live = (int)(batch - b0 < G ? batch - b0 : G);
    __syncthreads();

    // parity of the decisions P < 0 over this lane's checks of every layer: sets the codeword's unsat word
    auto syndrome = [&]() {
        unsigned bad = 0;
        for (int l = 0; l < pl.L; ++l) {
            const int c0 = pl.layer_ptr[l], S = pl.layer_ptr[l + 1] - c0, base = pl.entry_base[l];
            for (int jj = j; jj < S; jj += lpc) {
                const int dc = pl.deg[c0 + jj];
                unsigned par = 0;
                for (int k = 0; k < dc; ++k) par ^= P[pl.off[base + k * S + jj] >> 2] < 0.0f ? 1u : 0u;
                bad |= par;
            }
        }
        if (bad) f_unsat[g] = 1;                                // every writer writes 1
    };

    for (int it = 0; it < T; ++it) {
        if (ES && *f_live == 0) break;                          // uniform: written before the last barrier, read by all
        const bool work = mine && !(ES && f_frozen[g]);
        const bool first = it == 0;
        const float *bet = pl.beta_lay ? pl.beta_lay + (size_t)it * pl.entries : nullptr;
        const float *betp = pl.beta_lay ? pl.beta_lay + (size_t)(first ? 0 : it - 1) * pl.entries : nullptr;
        const float *oma = (FORM == FORM_OMS && AUX) ? pl.oms_lay + (size_t)it * pl.entries : nullptr;
        const float *omap = (FORM == FORM_OMS && AUX) ? pl.oms_lay + (size_t)(first ? 0 : it - 1) * pl.entries : nullptr;
        const float *thr = FORM == FORM_RCQ ? thresholds + (size_t)q_of_iter[it] * n_levels : nullptr;
        const float *thp = FORM == FORM_RCQ ? thresholds + (size_t)q_of_iter[first ? 0 : it - 1] * n_levels : nullptr;
        for (int l = 0; l < pl.L; ++l) {
            const int c0 = pl.layer_ptr[l], S = pl.layer_ptr[l + 1] - c0, base = pl.entry_base[l];
            if (work) {
                for (int jj = j; jj < S; jj += lpc) {
                    const int c = c0 + jj, dc = pl.deg[c];
                    if (dc == 0) continue;
                    const bool lone = dc == 1;                  // degree-1 check: min2 = min, product 1
                    const int e0 = base + jj;                   // entry of edge k: e0 + k * S
                    float m1 = inf_of<float>(), m2 = inf_of<float>();
                    unsigned par = 0;
                    if constexpr (FORM == FORM_RCQ) {
                        // the previous message of entry e: its code under the quantiser that produced it (+0 before any)
                        auto prev = [&](int e) {
                            const unsigned cold = Cd[e];
                            const float ro = first ? 0.0f : thp[cold & 0x7fu];
                            return flip_sign<float>(ro, cold >> 7);
                        };
                        for (int k = 0; k < dc; ++k) {
                            const int e = e0 + k * S;
                            const float u = __fsub_rn(P[pl.off[e] >> 2], prev(e));
                            const float a = __builtin_fabsf(u);
                            par ^= signbit_of<float>(u);
                            if (a < m1) { m2 = m1; m1 = a; }
                            else if (a < m2) { m2 = a; }
                        }
                        if (lone) m2 = m1;
                        for (int k = 0; k < dc; ++k) {
                            const int e = e0 + k * S;
                            const unsigned v = pl.off[e] >> 2;
                            const float u = __fsub_rn(P[v], prev(e));
                            const float a = __builtin_fabsf(u);
                            const float raw = (a == m1) ? m2 : m1;              // arg-min edge; ties make min2 == min1
                            const float w = flip_sign<float>(AUX ? __fmul_rn(bet[e], raw) : raw, par ^ signbit_of<float>(u));
                            const float mag = __builtin_fabsf(w);
                            float rec = thr[0];
                            unsigned lvl = 0;
                            for (int q = 1; q < n_levels; ++q) {
                                const bool ge = mag >= thr[q];
                                rec = ge ? thr[q] : rec;
                                lvl = ge ? (unsigned)q : lvl;
                            }
                            const unsigned neg = w < 0.0f ? 1u : 0u;
                            P[v] = __fadd_rn(u, flip_sign<float>(rec, neg));
                            Cd[e] = (uint8_t)(lvl | (neg << 7));
                        }
                    } else {
                        // the check record of the previous iteration and this lane's previous message from it
                        const unsigned m1o = Rw[c], m2o = Rw[m + c];
                        unsigned long long sgo = Rw[2 * m + c], ago = Rw[(2 + W) * m + c];
                        if (W == 2) {
                            sgo |= (unsigned long long)Rw[3 * m + c] << 32;
                            ago |= (unsigned long long)Rw[5 * m + c] << 32;
                        }
                        auto prev = [&](int e, int k) {
                            const float rawo = __uint_as_float(((ago >> k) & 1ull) ? m2o : m1o);
                            const float ro = lay_ms_msg<FORM>(rawo, (unsigned)((sgo >> k) & 1ull), betp[e], AUX ? omap[e] : 0.0f, lone);
                            return first ? 0.0f : ro;
                        };
                        for (int k = 0; k < dc; ++k) {
                            const int e = e0 + k * S;
                            const float u = __fsub_rn(P[pl.off[e] >> 2], prev(e, k));
                            const float a = __builtin_fabsf(u);
                            par ^= signbit_of<float>(u);
                            if (a < m1) { m2 = m1; m1 = a; }
                            else if (a < m2) { m2 = a; }
                        }
                        if (lone) m2 = m1;
                        unsigned long long sgn = 0, agn = 0;
                        for (int k = 0; k < dc; ++k) {
                            const int e = e0 + k * S;
                            const unsigned v = pl.off[e] >> 2;
                            const float u = __fsub_rn(P[v], prev(e, k));
                            const float a = __builtin_fabsf(u);
                            const bool arg = a == m1;                           // arg-min edge; ties make min2 == min1
                            const unsigned neg = par ^ signbit_of<float>(u);    // parity of the OTHER edges' sign bits
                            const float rn = lay_ms_msg<FORM>(arg ? m2 : m1, neg, bet[e], AUX ? oma[e] : 0.0f, lone);
                            P[v] = __fadd_rn(u, rn);                            // never an fma with the product inside rn
                            sgn |= (unsigned long long)neg << k;
                            agn |= (unsigned long long)(arg ? 1u : 0u) << k;
                        }
                        Rw[c] = __float_as_uint(m1);
                        Rw[m + c] = __float_as_uint(m2);
                        Rw[2 * m + c] = (unsigned)sgn;
                        Rw[(2 + W) * m + c] = (unsigned)agn;
                        if (W == 2) {
                            Rw[3 * m + c] = (unsigned)(sgn >> 32);
                            Rw[5 * m + c] = (unsigned)(agn >> 32);
                        }
                    }
                }
            }
            __syncthreads();                                    // the layer's barrier: every lane, whatever its codeword does
        }
        if (ES) {
            if (work) syndrome();
            __syncthreads();
            if (work && j == 0) {
                if (f_unsat[g] == 0) {                          // first zero-syndrome iteration latches
                    f_frozen[g] = 1;
                    f_iters[g] = it + 1;
                    atomicSub(f_live, 1);
                }
                f_unsat[g] = 0;
            }
            __syncthreads();
        }
    }

    // early stop: success = latched at a zero syndrome, iterations = that iteration (else T);
    // fixed T: success = the final syndrome is zero, iterations = T
    if (!ES) {
        if (mine) syndrome();
        __syncthreads();
    }
    if (mine && j == 0) {
        const bool ok = ES ? f_frozen[g] != 0 : f_unsat[g] == 0;
        if (iterations) iterations[b0 + g] = (ES && ok) ? f_iters[g] : T;
        if (success) success[b0 + g] = (uint8_t)(ok ? 1 : 0);
    }
    // outputs straight into the caller's rows, coalesced; a wave packs 64 consecutive decisions by ballot
    const int nbytes = (n + 7) / 8;
    for (int r = 0; r < G; ++r) {
        if (b0 + r >= batch) break;
        const float *row = blk_smem + (size_t)r * row_words;
        const size_t ob = (size_t)(b0 + r) * n;
        for (int j0 = tid - lane; j0 < n; j0 += NT) {
            const int x = j0 + lane;
            const bool in = x < n;
            const float v = in ? row[x] : 0.0f;
            const bool neg = in && v < 0.0f;
            if (in && posterior) __builtin_nontemporal_store(v, posterior + ob + x);
            if (in && bits) __builtin_nontemporal_store(neg ? 1 : 0, bits + ob + x);
            if (packed) {
                const unsigned long long mk = __ballot(neg);
                if (lane < 8 && j0 + 8 * lane < n) packed[(size_t)(b0 + r) * nbytes + (j0 >> 3) + lane] = (uint8_t)(mk >> (8 * lane));
            }
        }
    }
}

}  // namespace ldpc
