// ldpc_layered.hip -- LDS-resident layered RCQ decode (gfx950): lanes run over the EDGES of one check.
//
// Schedule: RCQMinSumDecoder._decode_layered as the reference executes it (rcq_decoder.py:281-350; its per-check
// message matrix is re-created for every check, so nothing is ever subtracted: posteriors accumulate every check's
// quantised message, check after check, inside and across iterations -- LDPC_SCHED_LAYERED_REF).  The walk over the
// checks is ONE dependent chain per codeword (check i+1 reads what check i wrote), m*T steps long; what can run in
// parallel is the batch and the edges of a check.  The streaming kernel (layered_rcq, ldpc_kernels.hip) keeps the
// posteriors in HBM and gives a lane a codeword: at 65536 codewords that is one wave per SIMD with a memory round trip
// per step.  Here a workgroup is ONE wave holding CW codewords' posterior vectors in LDS (4n bytes each):
//
//   lane = (row, t):  row = lane / LW  -> codeword of the wave,   t = lane % LW -> edge of the current check
//   LW = 2^k >= max check degree (1..64),  CW = 64 / LW codewords per wave (fewer when 4n*CW would exceed LDS)
//
// Per check: one ds_read per lane (posterior of the edge's variable), min1 / min2 / sign parity over the LW lanes by an
// XOR butterfly (DPP quad_perm / row_half_mirror / row_mirror inside 16 lanes, ds_swizzle / shuffle beyond), the
// quantise-reconstruct of sign * min-of-the-others per lane, one ds_write.  LDS instructions of a wave execute in order,
// so the chain needs no barrier; the plan entry of a lane (LDS byte offset of its variable, prefetched kPf checks ahead)
// is the only global-memory access of the loop.  LLRs come straight from the caller's rows and the outputs go straight
// back (no tile transposes, no workspace).  Several single-wave workgroups share a CU (five on the (1998,1512) code).
//
// What a step costs: ~36 instructions, half of them with a DPP operand (the butterfly), issued by ONE wave per SIMD -- a wave
// issues a dependent VALU instruction every ~9 cycles, a DPP one every ~16 with its hazard slot
// (tools/probes/valu_latency_probe.hip) -- so the quantise/select tail is scheduled by hand (ten instructions, no hazard
// padding) and the step is bounded by VALU time, not by the LDS round trip.
//
// Every row is read after the previous row's write.  Reading the next row one step early (exact where the rows share no
// variable, a DPP forward for the parity chain) was measured slower at full occupancy: (1998,1512), 65536 codewords, T = 10:
// in order 8.87-8.90 ms, early 9.23-9.25 ms -- a step is bounded by the VALU time of its ~19 DPP operations, not by the LDS
// round trip, and the in-order form's LDS waits are what the fifth wave of a CU fills.
//
// Arithmetic is that of layered_rcq (same helpers): results are identical to the streaming kernel's.
//
// layered_paper_lds (below): the same walk for LDPC_SCHED_LAYERED, the paper's schedule (previous message subtracted, optional
// beta), with each edge's message code kept in LDS beside the posteriors.
//
// layered_minsum_lds (below that): the same schedule with unquantised messages for the min-sum decoders (LDPC_C2V_NMS /
// LDPC_C2V_OMS), with a check record per check in LDS from which each lane recomputes its previous message.
#pragma once

#include "ldpc_kernels.hip"

namespace ldpc {

struct LayeredPlan {
    int n, m, lw, cw;              // lanes per check, codewords per wave
    int m_pad;                     // plan rows walked: m rounded up to a multiple of kLayPf with no-op rows (every lane at +inf)
    int has_deg1;                  // some check has exactly one edge (its entries carry bit 31)
    int zero0;                     // every quantiser reconstructs magnitude 0 as 0 (tau_0 == 0, the other thresholds > 0)
    int sorted;                    // tau_1 <= tau_2 <= ... under every quantiser
    int row_shift;                 // > 0: a codeword's LDS region is 2^row_shift bytes (its address is then offset | row bits: one
                                   // v_and_or_b32); 0: (n + 1) * 4 bytes, packed
    const uint32_t *off;           // [m_pad + 2 * kLayPf][lw]  bits 0..28: LDS byte offset (4 * variable) of the edge in lane t of check
                                   //          i (edges right-aligned, ascending variable order); lanes without an
                                   //          edge point at word n of the codeword's vector, which holds +inf for ever (it
                                   //          is neutral for min and parity, and inf + message = inf is written back);
                                   //          bit 29 (kLayDeg1Bit) on the entries of a degree-1 check ("min2 = min", :312-313);
                                   //          no-op rows up to m_pad (inf in, inf out), then 2 * kLayPf more that only the
                                   //          prefetch past the last check reads
    // LDPC_SCHED_LAYERED (layered_paper_lds) only:
    unsigned row_bytes;            // LDS bytes of one codeword: posteriors + the +inf word, then the codes
    unsigned code_off;             // byte offset of the codes inside a codeword's region: code of plan entry (i, t) at + i * lw + t
    const float *beta_lay;         // [T][m_pad + 2 * kLayPf][lw] beta_t of the edge in plan entry (i, t) (1 where none)
    // layered_minsum_lds: row_bytes / code_off describe the check records that take the place of the codes (one per plan row)
    const float *oms_lay;          // offset form with a check-side alpha table: a_t in plan order, as beta_lay; else NULL
};

constexpr int kLayPf = 4;          // plan entries in flight ahead of the check being processed (= the unroll of the walk)
constexpr uint32_t kLayOffMask = 0x1fffffffu;
constexpr uint32_t kLayDeg1Bit = 0x20000000u;

// LDS bytes of one codeword: n posteriors + the +inf word
__host__ __device__ inline size_t lay_row_bytes(int n) { return ((size_t)n + 1) * 4; }

template <int O>
__device__ __forceinline__ unsigned lay_xchg(unsigned v)
{
    // partner lane ^ O for a butterfly whose earlier steps ran in order (1, 2, 4, ...): after steps 1 and 2 the four lanes of
    // a quad agree, so "the other quad of my half row" may be ANY lane of it (row_half_mirror), likewise row_mirror for 8.
    // bound_ctrl: no `old` operand to materialise (every lane is active and every source lane exists)
    if constexpr (O == 1) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);        // quad_perm [1,0,3,2]
    else if constexpr (O == 2) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
    else if constexpr (O == 4) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true);  // row_half_mirror
    else if constexpr (O == 8) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true);  // row_mirror
    else if constexpr (O == 16) return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, (16 << 10) | 0x1f);
    else return (unsigned)__shfl_xor((int)v, 32, 64);
}

// One butterfly step on (min1, min2, XOR of the raw bit patterns).  Magnitudes are non-negative floats, so their BIT
// PATTERNS order like unsigned integers (+inf above every finite value): v_min_u32 / v_max_u32 take the exchanged operand
// through DPP directly and need no canonicalisation.  (A NaN input orders above +inf here; the float compares of the
// streaming kernel skip it -- results agree on every non-NaN input.)
template <int O, int LW>
__device__ __forceinline__ void lay_step(unsigned &m1, unsigned &m2, unsigned &par)
{
    if constexpr (O == 1 && O < LW) {                            // first step: min2 is still +inf on every lane
        const unsigned a = m1;
        m2 = max(a, lay_xchg<1>(a));
        m1 = min(a, lay_xchg<1>(a));
        par ^= lay_xchg<1>(par);
    } else if constexpr (O < LW) {
        const unsigned hi = max(m1, lay_xchg<O>(m1));            // each exchanged value has ONE use: folds into the DPP operand
        const unsigned lo2 = min(m2, lay_xchg<O>(m2));
        par ^= lay_xchg<O>(par);
        m1 = min(m1, lay_xchg<O>(m1));
        m2 = min(hi, lo2);                                       // second smallest of {m1, m2, o1, o2}; ties keep min2 == min1
    }
}
template <int O, int LW>
__device__ __forceinline__ void lay_step_xor(unsigned &x)
{
    if constexpr (O < LW) x ^= lay_xchg<O>(x);
}

__device__ __forceinline__ float lay_lds_ld(unsigned byte_off)
{
    return *(__attribute__((address_space(3))) const float *)(size_t)byte_off;
}
__device__ __forceinline__ void lay_lds_st(unsigned byte_off, float v)
{
    *(__attribute__((address_space(3))) float *)(size_t)byte_off = v;
}
__device__ __forceinline__ unsigned lay_lds_ld8(unsigned byte_off)
{
    return *(__attribute__((address_space(3))) const uint8_t *)(size_t)byte_off;
}
__device__ __forceinline__ void lay_lds_st8(unsigned byte_off, unsigned v)
{
    *(__attribute__((address_space(3))) uint8_t *)(size_t)byte_off = (uint8_t)v;
}

// NL: compile-time level count (4 = bc 3), 0 = run-time (up to 8 in registers, more from global memory)
// ES: early stop (per-iteration syndrome, frozen codewords keep their posteriors); D1: the code has degree-1 checks;
// Z0: magnitude 0 reconstructs to 0 under every quantiser -- the message sign is then the parity of the other signs without
//     the reference's "w < 0" test (it differs only in the sign of an exact zero message, which no later operation observes
//     as a value: x + (+-0) == x, |.|, the compares; same argument as ldpc_resident.hip's per-check quantisation)
// SORTED (NL = 4): tau_1 <= tau_2 <= tau_3 -- the level is then found by a two-deep select tree, and BOTH candidate outputs
//     (reconstruction of min1 and of min2) are formed side by side right after the butterfly; the lane only picks.  On one
//     wave a dependent VALU instruction issues every ~9 cycles and a compare -> select pair costs ~21
//     (tools/probes/valu_latency_probe.hip), so the depth of this tail, not its instruction count, is what a step costs.
template <int LW, int NL, bool ES, bool D1, bool Z0, bool SORTED = false, bool P2 = false>
__global__ __launch_bounds__(kWave) void layered_lds(LayeredPlan pl, const float *__restrict__ llr, long long batch,
                                                     const float *__restrict__ thresholds, int n_levels,
                                                     const int *__restrict__ q_of_iter, int T,
                                                     int *__restrict__ bits, float *__restrict__ posterior,
                                                     int *__restrict__ iterations, uint8_t *__restrict__ success,
                                                     uint8_t *__restrict__ packed)
{
    extern __shared__ __align__(16) unsigned char lay_smem[];       // the only LDS object: posteriors start at offset 0
    if (__builtin_amdgcn_groupstaticsize() != 0) __builtin_trap();  // lay_lds_ld / lay_lds_st rely on that (folds away)
    const int lane = threadIdx.x;
    const int n = pl.n, m = pl.m_pad, cw = pl.cw;                  // m: plan rows incl. the no-op padding
    const int row = lane / LW, t = lane % LW;
    const long long b0 = (long long)blockIdx.x * cw;
    // lane groups beyond the wave's codewords (cw < 64 / LW: large n) SHADOW the last one: same reads, same state, the same
    // values written to the same addresses -- they must take every decision (frozen, latch) exactly as the group they shadow
    const int row_eff = min(row, cw - 1);
    const bool row_live = b0 + row_eff < batch;                     // this lane's codeword exists (padding rows of the last wave do not)
    const unsigned row_words = P2 ? (1u << pl.row_shift) / 4u : (unsigned)n + 1u;
    const unsigned row_base = (unsigned)row_eff * row_words * 4u;
    // LDS address of a plan entry: P2 -> the row bits are disjoint from the offset bits, mask and combine are one instruction
    auto lds_addr = [&](uint32_t o) { return P2 ? ((o & kLayOffMask) | row_base) : (row_base + (o & kLayOffMask)); };

    // LLRs: the caller's rows, coalesced (all 64 lanes over one row at a time); "posteriors = llr.clone()" (:288)
    for (int r = 0; r < cw; ++r) {
        const bool have = b0 + r < batch;
        const float *src = llr + (size_t)(b0 + r) * n;
        for (int j = lane; j < n; j += kWave)
            lay_lds_st(((unsigned)r * row_words + (unsigned)j) * 4u, have ? __builtin_nontemporal_load(src + j) : 1.0f);
        if (lane == 0) lay_lds_st(((unsigned)r * row_words + (unsigned)n) * 4u, inf_of<float>());
    }
    asm volatile("" ::: "memory");

    unsigned frozen = row_live ? 0u : 1u;                           // row-uniform: this lane's codeword has stopped (or is padding)
    int my_iters = T;
    const uint32_t *plan = pl.off + t;

    // syndrome of the current posteriors: 1 when some check of this lane's codeword is unsatisfied (row-uniform);
    // nothing depends on the previous check here, so the loop pipelines (hard decision = "posterior < 0", :341;
    // the +inf word of a lane without an edge contributes 0)
    auto syndrome = [&]() {
        unsigned unsat = 0;
#pragma unroll 4
        for (int i = 0; i < m; ++i) {
            const uint32_t o = plan[(size_t)i * LW];
            unsigned s = lay_lds_ld(lds_addr(o)) < 0.0f ? 1u : 0u;
            lay_step_xor<1, LW>(s); lay_step_xor<2, LW>(s); lay_step_xor<4, LW>(s);
            lay_step_xor<8, LW>(s); lay_step_xor<16, LW>(s); lay_step_xor<32, LW>(s);
            unsat |= s;
        }
        return unsat & 1u;
    };

    for (int it = 0; it < T; ++it) {
        if (ES && __ballot(frozen == 0u) == 0ull) break;
        const float *thr = thresholds + (size_t)q_of_iter[it] * n_levels;
        float th[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (NL > 0) th[q] = q < NL ? thr[q] : 0.0f;
            else th[q] = (q < n_levels) ? thr[q] : __builtin_nanf("");
            asm volatile("" : "+v"(th[q]));                         // in VGPRs for the whole walk (a select takes one scalar operand: its mask)
        }
        // one check: o = this lane's plan entry.  The second argument (its entry of the NEXT row) is not read; the call
        // still passes it because dropping it changes the code the compiler generates for this kernel.
        auto step = [&](uint32_t o, uint32_t /*next*/) {
            const unsigned addr = lds_addr(o);
            const float x = lay_lds_ld(addr);                       // in order: after the previous row's write
            const unsigned xb = __float_as_uint(x), a = xb & 0x7fffffffu;
            unsigned m1 = a, m2 = 0x7f800000u, par = xb;
            lay_step<1, LW>(m1, m2, par); lay_step<2, LW>(m1, m2, par); lay_step<4, LW>(m1, m2, par);
            lay_step<8, LW>(m1, m2, par); lay_step<16, LW>(m1, m2, par); lay_step<32, LW>(m1, m2, par);
            if (D1 && (o & kLayDeg1Bit)) m2 = m1;                   // degree-1 check: "min2_val = min_val" (:312-313)
            float msg;
            if constexpr (NL == 4 && SORTED && Z0) {
                // raw = min over the OTHER edges (arg-min edge takes min2; ties make min2 == min1); rec = tau[last q with raw >=
                // tau_q]; sorted thresholds: c3 => c2 => c1, so rec = c2 ? (c3 ? tau3 : tau2) : (c1 ? tau1 : tau0).  Scheduled by
                // hand -- ten instructions, every compare two or more instructions ahead of the select that reads its mask; the
                // compiler routes every compare/select pair through vcc with an s_nop each.  (One wave issues an instruction
                // every 6-9 cycles whatever it is -- tools/probes/valu_latency_probe.hip -- so a step costs its instruction
                // COUNT: forming both candidates side by side was measured slower than this.)
                float rec, raw, lo, hi;
                unsigned long long ca, cb;
                unsigned sgn;                                        // par ^ x: formed inside the block, in a hazard slot
                asm("v_cmp_eq_u32_e32 vcc, %[a], %[m1]\n\t"
                    "v_xor_b32_e32 %[sgn], %[par], %[xb]\n\t"
                    "s_nop 0\n\t"
                    "v_cndmask_b32_e32 %[raw], %[m1], %[m2], vcc\n\t"
                    "v_cmp_le_f32_e64 %[ca], %[t1], %[raw]\n\t"
                    "v_cmp_le_f32_e64 %[cb], %[t3], %[raw]\n\t"
                    "v_cmp_le_f32_e32 vcc, %[t2], %[raw]\n\t"
                    "v_cndmask_b32_e64 %[lo], %[t0], %[t1], %[ca]\n\t"
                    "v_cndmask_b32_e64 %[hi], %[t2], %[t3], %[cb]\n\t"
                    "v_cndmask_b32_e32 %[rec], %[lo], %[hi], vcc"
                    : [rec] "=v"(rec), [raw] "=&v"(raw), [lo] "=&v"(lo), [hi] "=&v"(hi), [sgn] "=&v"(sgn), [ca] "=&s"(ca), [cb] "=&s"(cb)
                    : [t0] "v"(th[0]), [t1] "v"(th[1]), [t2] "v"(th[2]), [t3] "v"(th[3]), [m1] "v"(m1), [m2] "v"(m2), [a] "v"(a),
                      [par] "v"(par), [xb] "v"(xb)
                    : "vcc");
                msg = __uint_as_float(__builtin_amdgcn_bitop3_b32(__float_as_uint(rec), sgn, 0x80000000u, 0x78));   // a ^ (b & c)
            } else {
            const float raw = __uint_as_float((a == m1) ? m2 : m1);  // arg-min edge; ties make min2 == min1
            float rec;
            if constexpr (NL > 0) {
                rec = th[0];
#pragma unroll
                for (int q = 1; q < NL; ++q) rec = (raw >= th[q]) ? th[q] : rec;
            } else if (n_levels <= 8) {
                rec = th[0];
#pragma unroll
                for (int q = 1; q < 8; ++q) rec = (raw >= th[q]) ? th[q] : rec;      // NaN padding never matches
            } else {
                rec = thr[0];
                for (int q = 1; q < n_levels; ++q) rec = (raw >= thr[q]) ? thr[q] : rec;
            }
            // message = (1 - 2*sign_bit) * tau[level] (:107-119), sign_bit = (sign * raw < 0): the parity of the OTHER edges'
            // sign bits (bit 31 of par ^ x), counted only for a non-zero magnitude
            if constexpr (Z0) {
                msg = __uint_as_float(__builtin_amdgcn_bitop3_b32(__float_as_uint(rec), par ^ xb, 0x80000000u, 0x78));   // a ^ (b & c)
            } else {
                const unsigned neg = (raw > 0.0f) ? ((par ^ xb) & 0x80000000u) : 0u;
                msg = __uint_as_float(__float_as_uint(rec) ^ neg);
            }
            }
            float upd = x + msg;                                    // "posteriors[j] += c2v_messages[i, j]" (:337-338)
            if (ES) upd = frozen ? x : upd;                         // a stopped codeword keeps its posteriors
            lay_lds_st(addr, upd);
        };
        // Plan entries are requested a group ahead: rows 1.. of the NEXT group, and row 0 of the group after it.
        // m is a multiple of kLayPf and 2 * kLayPf more rows follow: no bounds tests.
        uint32_t cur[kLayPf], nxt[kLayPf], nn0;
#pragma unroll
        for (int k = 0; k < kLayPf; ++k) cur[k] = plan[(size_t)k * LW];
        nxt[0] = plan[(size_t)kLayPf * LW];
        for (int i0 = 0; i0 < m; i0 += kLayPf) {
            const uint32_t *nx = plan + (size_t)(i0 + kLayPf) * LW;
#pragma unroll
            for (int k = 1; k < kLayPf; ++k) nxt[k] = nx[(size_t)k * LW];
            nn0 = nx[(size_t)kLayPf * LW];
#pragma unroll
            for (int k = 0; k < kLayPf; ++k) step(cur[k], k + 1 < kLayPf ? cur[k + 1] : nxt[0]);
#pragma unroll
            for (int k = 0; k < kLayPf; ++k) cur[k] = nxt[k];
            nxt[0] = nn0;
        }
        if (ES) {
            const unsigned unsat = syndrome();
            if (frozen == 0u && unsat == 0u) { frozen = 1u; my_iters = it + 1; }      // first zero-syndrome iteration latches (:344-345)
        }
    }
    asm volatile("" ::: "memory");

    // early stop: success = latched at a zero syndrome, iterations = that iteration (else T, :348-349);
    // fixed T: success = the final syndrome is zero, iterations = T
    unsigned ok;
    if (ES) ok = (row_live && frozen != 0u) ? 1u : 0u;
    else ok = syndrome() == 0u ? 1u : 0u;
    if (row_live && row < cw && t == 0) {
        if (iterations) iterations[b0 + row] = (ES && ok) ? my_iters : T;
        if (success) success[b0 + row] = (uint8_t)ok;
    }
    // outputs straight into the caller's rows, coalesced
    const int nbytes = (n + 7) / 8;
    for (int r = 0; r < cw; ++r) {
        if (b0 + r >= batch) break;
        const size_t ob = (size_t)(b0 + r) * n;
        for (int j0 = 0; j0 < n; j0 += kWave) {
            const int j = j0 + lane;
            const bool in = j < n;
            const float v = in ? lay_lds_ld(((unsigned)r * row_words + (unsigned)j) * 4u) : 0.0f;
            const bool neg = in && v < 0.0f;
            if (in && posterior) __builtin_nontemporal_store(v, posterior + ob + j);
            if (in && bits) __builtin_nontemporal_store(neg ? 1 : 0, bits + ob + j);
            if (packed) {
                const unsigned long long mk = __ballot(neg);
                if (lane < 8 && j0 + 8 * lane < n) packed[(size_t)(b0 + r) * nbytes + (j0 >> 3) + lane] = (uint8_t)(mk >> (8 * lane));
            }
        }
    }
}

// ---- the paper's layered schedule (LDPC_SCHED_LAYERED): RCQMinSumDecoder(layered="paper") and
// WeightedRCQDecoder(layered="paper").  Same walk, lanes and butterfly as layered_lds; what is added is each edge's
// previous message, kept as its 1-byte code in LDS next to the codeword's posteriors (one byte per PLAN entry, i.e. per
// lane of each check row: lanes without an edge own a byte nobody else reads).  Per check, lane (row, t) on edge e = (c, v):
//   u      = P_v - Q_{t-1}^{-1}(R_e)                         (the code was written in the previous iteration; 0 before any)
//   min1 / min2 / parity over the u of the check             (butterfly on the u bit patterns, as layered_lds)
//   w      = +-(beta_t[slot(e)] * min_others)                (WB; the flooding W-RCQ product, sign = parity of the others)
//   R_e    = Q_t(w),  P_v = u + Q_t^{-1}(R_e)
// The codes in LDS carry level | sign << 7 (the reconstruction is sign-flipped tau[level]); 0 initially, which reconstructs
// to +0 under the all-zero "previous" table of iteration 0: x - (+0) == x for every x, -0 included.
// A frozen codeword (early stop) writes back what it read: posterior and code.  Arithmetic and conventions are those of
// layered_rcq<VEC, true>: results are identical to the streaming kernel's.
// NL: compile-time level count (4 = bc 3), 0 = run-time (up to 8 in registers, more from global memory); WB: weighted.
template <int LW, int NL, bool ES, bool WB>
__global__ __launch_bounds__(kWave) void layered_paper_lds(LayeredPlan pl, const float *__restrict__ llr, long long batch,
                                                           const float *__restrict__ thresholds, int n_levels,
                                                           const int *__restrict__ q_of_iter, int T,
                                                           int *__restrict__ bits, float *__restrict__ posterior,
                                                           int *__restrict__ iterations, uint8_t *__restrict__ success,
                                                           uint8_t *__restrict__ packed)
{
    extern __shared__ __align__(16) unsigned char lay_smem[];       // the only LDS object: codeword regions start at offset 0
    if (__builtin_amdgcn_groupstaticsize() != 0) __builtin_trap();
    const int lane = threadIdx.x;
    const int n = pl.n, m = pl.m_pad, cw = pl.cw;
    const int row = lane / LW, t = lane % LW;
    const long long b0 = (long long)blockIdx.x * cw;
    const int row_eff = min(row, cw - 1);                           // shadow lanes: see layered_lds
    const bool row_live = b0 + row_eff < batch;
    const unsigned row_bytes = pl.row_bytes;
    const unsigned row_base = (unsigned)row_eff * row_bytes;
    const unsigned code_base = row_base + pl.code_off + (unsigned)t;

    for (int r = 0; r < cw; ++r) {
        const bool have = b0 + r < batch;
        const float *src = llr + (size_t)(b0 + r) * n;
        const unsigned rb = (unsigned)r * row_bytes;
        for (int j = lane; j < n; j += kWave)
            lay_lds_st(rb + (unsigned)j * 4u, have ? __builtin_nontemporal_load(src + j) : 1.0f);
        if (lane == 0) lay_lds_st(rb + (unsigned)n * 4u, inf_of<float>());
        for (unsigned k = pl.code_off + 4u * (unsigned)lane; k < row_bytes; k += 4u * kWave) lay_lds_st(rb + k, 0.0f);   // codes: none
    }
    asm volatile("" ::: "memory");

    unsigned frozen = row_live ? 0u : 1u;
    int my_iters = T;
    const uint32_t *plan = pl.off + t;
    const size_t plan_rows = (size_t)m + 2 * kLayPf;

    auto syndrome = [&]() {
        unsigned unsat = 0;
#pragma unroll 4
        for (int i = 0; i < m; ++i) {
            const uint32_t o = plan[(size_t)i * LW];
            unsigned s = lay_lds_ld(row_base + (o & kLayOffMask)) < 0.0f ? 1u : 0u;
            lay_step_xor<1, LW>(s); lay_step_xor<2, LW>(s); lay_step_xor<4, LW>(s);
            lay_step_xor<8, LW>(s); lay_step_xor<16, LW>(s); lay_step_xor<32, LW>(s);
            unsat |= s;
        }
        return unsat & 1u;
    };

    for (int it = 0; it < T; ++it) {
        if (ES && __ballot(frozen == 0u) == 0ull) break;
        const float *thr = thresholds + (size_t)q_of_iter[it] * n_levels;
        const float *thp = thresholds + (size_t)q_of_iter[it > 0 ? it - 1 : 0] * n_levels;
        // thresholds of this iteration (c*) and of the previous one (p*, 0 at it 0) as SEPARATE registers, looked up by a select
        // tree on the level bits: over an array, "lvl == q ? t[q] : ..." is folded into an indexed load, which puts the array in
        // memory (promoted to static LDS -- the kernel must have none)
        float c0, c1, c2, c3, c4, c5, c6, c7, p0, p1, p2, p3, p4, p5, p6, p7;
        {
            const int nl = NL > 0 ? NL : n_levels;
            const float pad = NL > 0 ? 0.0f : __builtin_nanf("");  // never matched by a compare
            auto ld = [&](const float *tb, int q, float none) { return q < nl && q < 8 ? tb[q] : none; };
            c0 = ld(thr, 0, pad); c1 = ld(thr, 1, pad); c2 = ld(thr, 2, pad); c3 = ld(thr, 3, pad);
            c4 = ld(thr, 4, pad); c5 = ld(thr, 5, pad); c6 = ld(thr, 6, pad); c7 = ld(thr, 7, pad);
            auto lp = [&](int q) { return it > 0 ? ld(thp, q, 0.0f) : 0.0f; };
            p0 = lp(0); p1 = lp(1); p2 = lp(2); p3 = lp(3); p4 = lp(4); p5 = lp(5); p6 = lp(6); p7 = lp(7);
            asm volatile("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7));
            asm volatile("" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7));
        }
        auto sel4 = [](unsigned l, float a0, float a1, float a2, float a3) { return (l & 2u) ? ((l & 1u) ? a3 : a2) : ((l & 1u) ? a1 : a0); };
        const float *bet = WB ? pl.beta_lay + (size_t)it * plan_rows * LW + t : nullptr;
        auto step = [&](uint32_t o, float b, int i) {
            const unsigned addr = row_base + (o & kLayOffMask), caddr = code_base + (unsigned)i * LW;
            const float x = lay_lds_ld(addr);
            const unsigned cold = lay_lds_ld8(caddr), lvo = cold & 0x7fu;
            float ro;                                               // reconstruction of the previous code
            if constexpr (NL > 0) {
                static_assert(NL <= 4, "compile-time level counts: 4");
                ro = sel4(lvo, p0, p1, p2, p3);
            } else if (n_levels <= 8) {
                ro = (lvo & 4u) ? sel4(lvo, p4, p5, p6, p7) : sel4(lvo, p0, p1, p2, p3);
            } else {
                ro = it > 0 ? thp[lvo] : 0.0f;                      // lvo < n_levels: written by this kernel
            }
            const float u = x - flip_sign<float>(ro, cold >> 7);    // "subtract previous C2V messages" (:300-302)
            const unsigned ub = __float_as_uint(u), a = ub & 0x7fffffffu;
            unsigned m1 = a, m2 = 0x7f800000u, par = ub;
            lay_step<1, LW>(m1, m2, par); lay_step<2, LW>(m1, m2, par); lay_step<4, LW>(m1, m2, par);
            lay_step<8, LW>(m1, m2, par); lay_step<16, LW>(m1, m2, par); lay_step<32, LW>(m1, m2, par);
            if (o & kLayDeg1Bit) m2 = m1;                           // degree-1 check: min2 = min
            const float raw = __uint_as_float((a == m1) ? m2 : m1); // arg-min edge; ties make min2 == min1
            const float w = flip_sign<float>(WB ? b * raw : raw, (par ^ ub) >> 31);
            const float mag = __builtin_fabsf(w);
            float rec;
            unsigned lvl = 0;
            if constexpr (NL > 0) {
                lvl = mag >= c1 ? 1u : lvl; lvl = mag >= c2 ? 2u : lvl; lvl = mag >= c3 ? 3u : lvl;
                rec = sel4(lvl, c0, c1, c2, c3);
            } else if (n_levels <= 8) {
                lvl = mag >= c1 ? 1u : lvl; lvl = mag >= c2 ? 2u : lvl; lvl = mag >= c3 ? 3u : lvl; lvl = mag >= c4 ? 4u : lvl;
                lvl = mag >= c5 ? 5u : lvl; lvl = mag >= c6 ? 6u : lvl; lvl = mag >= c7 ? 7u : lvl;
                rec = (lvl & 4u) ? sel4(lvl, c4, c5, c6, c7) : sel4(lvl, c0, c1, c2, c3);
            } else {
                rec = thr[0];
                for (int q = 1; q < n_levels; ++q) { const bool ge = mag >= thr[q]; rec = ge ? thr[q] : rec; lvl = ge ? (unsigned)q : lvl; }
            }
            const unsigned neg = w < 0.0f ? 1u : 0u;                // sign(w) < 0 (rcq_decoder.py:88)
            float upd = u + flip_sign<float>(rec, neg);
            unsigned cnew = lvl | (neg << 7);
            if (ES && frozen) { upd = x; cnew = cold; }            // a stopped codeword keeps posterior and code
            lay_lds_st(addr, upd);
            lay_lds_st8(caddr, cnew);
        };
        // plan entries (and betas) a group ahead, as layered_lds: m is a multiple of kLayPf, 2 * kLayPf rows follow
        uint32_t cur[kLayPf], nxt[kLayPf];
        float bc[kLayPf], bn[kLayPf];
#pragma unroll
        for (int k = 0; k < kLayPf; ++k) {
            cur[k] = plan[(size_t)k * LW];
            bc[k] = WB ? bet[(size_t)k * LW] : 1.0f;
        }
        for (int i0 = 0; i0 < m; i0 += kLayPf) {
#pragma unroll
            for (int k = 0; k < kLayPf; ++k) {
                nxt[k] = plan[(size_t)(i0 + kLayPf + k) * LW];
                bn[k] = WB ? bet[(size_t)(i0 + kLayPf + k) * LW] : 1.0f;
            }
#pragma unroll
            for (int k = 0; k < kLayPf; ++k) step(cur[k], bc[k], i0 + k);
#pragma unroll
            for (int k = 0; k < kLayPf; ++k) { cur[k] = nxt[k]; bc[k] = bn[k]; }
        }
        if (ES) {
            const unsigned unsat = syndrome();
            if (frozen == 0u && unsat == 0u) { frozen = 1u; my_iters = it + 1; }
        }
    }
    asm volatile("" ::: "memory");

    unsigned ok;
    if (ES) ok = (row_live && frozen != 0u) ? 1u : 0u;
    else ok = syndrome() == 0u ? 1u : 0u;
    if (row_live && row < cw && t == 0) {
        if (iterations) iterations[b0 + row] = (ES && ok) ? my_iters : T;
        if (success) success[b0 + row] = (uint8_t)ok;
    }
    const int nbytes = (n + 7) / 8;
    for (int r = 0; r < cw; ++r) {
        if (b0 + r >= batch) break;
        const size_t ob = (size_t)(b0 + r) * n;
        for (int j0 = 0; j0 < n; j0 += kWave) {
            const int j = j0 + lane;
            const bool in = j < n;
            const float v = in ? lay_lds_ld((unsigned)r * row_bytes + (unsigned)j * 4u) : 0.0f;
            const bool neg = in && v < 0.0f;
            if (in && posterior) __builtin_nontemporal_store(v, posterior + ob + j);
            if (in && bits) __builtin_nontemporal_store(neg ? 1 : 0, bits + ob + j);
            if (packed) {
                const unsigned long long mk = __ballot(neg);
                if (lane < 8 && j0 + 8 * lane < n) packed[(size_t)(b0 + r) * nbytes + (j0 >> 3) + lane] = (uint8_t)(mk >> (8 * lane));
            }
        }
    }
}

// ---- layered schedule of the min-sum decoders (LDPC_SCHED_LAYERED with LDPC_C2V_NMS / LDPC_C2V_OMS): the unquantised
// baseline of layered_paper_lds.  Same walk, lanes, butterfly, plan prefetch and epilogue.  Per check, lane (row, t) on
// edge e = (c, v):
//   u     = P_v - R_e                                         (R_e: the edge's message of the previous iteration, +0 before any)
//   m1 / m2 / parity over the u of the check                  (butterfly on the bit patterns of |u|)
//   raw   = (|u| == m1) ? m2 : m1 ;  s = parity of the OTHER edges' sign bits
//   NMS:  r = +-(beta_t[slot(e)] * raw)                       OMS:  r = raw == 0 ? +0 : +-(relu(raw - beta_t) - a_t)
//   P_v   = u + r ;  R_e = r
// What is kept of R is not an fp32 word per plan entry (31 KB per codeword on the (1998,1512) code) but the CHECK RECORD
// of the iteration that produced the messages: m1, m2, one sign bit and one "was the arg-min" bit per lane of the row --
// 16 bytes per check for LW <= 32 { m1, m2, signs, argmins }, 24 for LW = 64 { m1, m2, signs lo, hi, argmins lo, hi } --
// read by all lanes of a row at one address.  The lane recomputes R_e from the record with beta_{t-1} (a_{t-1}) of its
// plan entry: the same operands through the same single operation give the same bits as a stored value would.
//
// Why the results equal a scalar restatement bit for bit:
//   no contraction -- every step (x - R, beta * raw, raw - beta, relu - a, u + r) is ONE rounded operation on values that
//     involve no summation order; the one hazard is u + (beta * raw) becoming an fma, hence __fmul_rn / __fadd_rn;
//   signs and zeros -- with sign bits in place of sgn(), "the product over the others is 0" holds exactly when raw == 0.
//     NMS: the message is then +-0 either way, which no later operation observes as a value (x + (+-0) == x, |.|, the
//     compares; a zero's own sign bit never enters its own message).  OMS: the message is forced to +0, otherwise -+a of
//     the offset would leak out -- except on a degree-1 check, whose edge has no others (product 1, raw = its own |u|).
// Lanes without an edge (they hold the +inf word) carry no message: R = r = 0, so inf - 0 + 0 = inf is written back (a
// message recomputed from an all-inf row would be inf, and inf - inf poisons the word).  LLRs must be finite.
// A frozen codeword (early stop) writes back what it read: posterior and record.  Results are identical to the streaming
// kernel's (layered_minsum, ldpc_kernels.hip), which keeps R_e itself.
// OA: the decoder has a check-side alpha table (FORM_OMS only; a = 0 without one)
template <int LW, int FORM, bool ES, bool OA>
__global__ __launch_bounds__(kWave) void layered_minsum_lds(LayeredPlan pl, const float *__restrict__ llr, long long batch, int T,
                                                            int *__restrict__ bits, float *__restrict__ posterior,
                                                            int *__restrict__ iterations, uint8_t *__restrict__ success,
                                                            uint8_t *__restrict__ packed)
{
    static_assert(FORM == FORM_NMS || FORM == FORM_OMS, "min-sum forms");
    extern __shared__ __align__(16) unsigned char lay_smem[];       // the only LDS object: codeword regions start at offset 0
    if (__builtin_amdgcn_groupstaticsize() != 0) __builtin_trap();
    constexpr unsigned kRec = LW <= 32 ? 16u : 24u;                 // bytes of a check record
    constexpr unsigned kMaskOff = 8u, kArgOff = LW <= 32 ? 12u : 16u;
    const int lane = threadIdx.x;
    const int n = pl.n, m = pl.m_pad, cw = pl.cw;
    const int row = lane / LW, t = lane % LW;
    const long long b0 = (long long)blockIdx.x * cw;
    const int row_eff = min(row, cw - 1);                           // shadow lanes: see layered_lds
    const bool row_live = b0 + row_eff < batch;
    const unsigned row_bytes = pl.row_bytes;
    const unsigned row_base = (unsigned)row_eff * row_bytes;
    const unsigned rec_base = row_base + pl.code_off;               // record of plan row i at + i * kRec
    const unsigned none_off = (unsigned)n * 4u;                     // plan offset of a lane without an edge
    const unsigned word = LW <= 32 ? 0u : 4u * ((unsigned)t >> 5), bit = (unsigned)t & 31u;

    for (int r = 0; r < cw; ++r) {
        const bool have = b0 + r < batch;
        const float *src = llr + (size_t)(b0 + r) * n;
        const unsigned rb = (unsigned)r * row_bytes;
        for (int j = lane; j < n; j += kWave)
            lay_lds_st(rb + (unsigned)j * 4u, have ? __builtin_nontemporal_load(src + j) : 1.0f);
        if (lane == 0) lay_lds_st(rb + (unsigned)n * 4u, inf_of<float>());
        for (unsigned k = pl.code_off + 4u * (unsigned)lane; k < row_bytes; k += 4u * kWave) lay_lds_st(rb + k, 0.0f);   // records: none
    }
    asm volatile("" ::: "memory");

    unsigned frozen = row_live ? 0u : 1u;
    int my_iters = T;
    const uint32_t *plan = pl.off + t;
    const size_t plan_rows = (size_t)m + 2 * kLayPf;

    auto syndrome = [&]() {
        unsigned unsat = 0;
#pragma unroll 4
        for (int i = 0; i < m; ++i) {
            const uint32_t o = plan[(size_t)i * LW];
            unsigned s = lay_lds_ld(row_base + (o & kLayOffMask)) < 0.0f ? 1u : 0u;
            lay_step_xor<1, LW>(s); lay_step_xor<2, LW>(s); lay_step_xor<4, LW>(s);
            lay_step_xor<8, LW>(s); lay_step_xor<16, LW>(s); lay_step_xor<32, LW>(s);
            unsat |= s;
        }
        return unsat & 1u;
    };

    for (int it = 0; it < T; ++it) {
        if (ES && __ballot(frozen == 0u) == 0ull) break;
        const bool first = it == 0;                                 // no record yet: R = +0
        const float *bet = pl.beta_lay + (size_t)it * plan_rows * LW + t;
        const float *betp = pl.beta_lay + (size_t)(first ? 0 : it - 1) * plan_rows * LW + t;
        const float *oma = OA ? pl.oms_lay + (size_t)it * plan_rows * LW + t : nullptr;
        const float *omap = OA ? pl.oms_lay + (size_t)(first ? 0 : it - 1) * plan_rows * LW + t : nullptr;
        auto step = [&](uint32_t o, float b, float bp, float a, float ap, int i) {
            const unsigned po = o & kLayOffMask, addr = row_base + po, raddr = rec_base + (unsigned)i * kRec;
            const bool edge = po != none_off;
            const float x = lay_lds_ld(addr);
            const unsigned m1o = __float_as_uint(lay_lds_ld(raddr)), m2o = __float_as_uint(lay_lds_ld(raddr + 4u));
            const unsigned sgo = __float_as_uint(lay_lds_ld(raddr + kMaskOff + word));
            const unsigned ago = __float_as_uint(lay_lds_ld(raddr + kArgOff + word));
            // the previous message, from the record: raw of this lane, its sign, beta_{t-1} (a_{t-1}) of its entry
            const float rawo = __uint_as_float(((ago >> bit) & 1u) ? m2o : m1o);
            const bool lone = (o & kLayDeg1Bit) != 0u;              // degree-1 check: no other edge, its product is 1
            float ro = lay_ms_msg<FORM>(rawo, (sgo >> bit) & 1u, bp, ap, lone);
            ro = (first || !edge) ? 0.0f : ro;
            const float u = __fsub_rn(x, ro);
            const unsigned ub = __float_as_uint(u), au = ub & 0x7fffffffu;
            unsigned m1 = au, m2 = 0x7f800000u, par = ub;
            lay_step<1, LW>(m1, m2, par); lay_step<2, LW>(m1, m2, par); lay_step<4, LW>(m1, m2, par);
            lay_step<8, LW>(m1, m2, par); lay_step<16, LW>(m1, m2, par); lay_step<32, LW>(m1, m2, par);
            if (lone) m2 = m1;                                      // degree-1 check: min2 = min
            const bool arg = au == m1;                              // arg-min edge; ties make min2 == min1
            const unsigned neg = (par ^ ub) >> 31;                  // parity of the OTHER edges' sign bits
            float rn = lay_ms_msg<FORM>(__uint_as_float(arg ? m2 : m1), neg, b, a, lone);
            rn = edge ? rn : 0.0f;
            float upd = __fadd_rn(u, rn);                           // never an fma with the product inside rn
            // the row's bits of the two ballots (shadow rows hold the bits of the row they shadow at their own position)
            const unsigned long long sb = __ballot(neg != 0u), ab = __ballot(arg);
            unsigned sgn, agn;
            if constexpr (LW == 64) {
                sgn = t < 32 ? (unsigned)sb : (unsigned)(sb >> 32);
                agn = t < 32 ? (unsigned)ab : (unsigned)(ab >> 32);
            } else {
                constexpr unsigned keep = LW == 32 ? 0xffffffffu : ((1u << LW) - 1u);
                sgn = (unsigned)(sb >> (row * LW)) & keep;
                agn = (unsigned)(ab >> (row * LW)) & keep;
            }
            if (ES && frozen) { upd = x; m1 = m1o; m2 = m2o; sgn = sgo; agn = ago; }   // a stopped codeword keeps posterior and record
            lay_lds_st(addr, upd);
            // lanes 0 and 32 of the row write the record (LW = 64: each its half of the masks; the same m1 / m2 twice)
            if (bit == 0u) {
                lay_lds_st(raddr, __uint_as_float(m1));
                lay_lds_st(raddr + 4u, __uint_as_float(m2));
                lay_lds_st(raddr + kMaskOff + word, __uint_as_float(sgn));
                lay_lds_st(raddr + kArgOff + word, __uint_as_float(agn));
            }
        };
        // plan entries and weights a group ahead, as layered_paper_lds: m is a multiple of kLayPf, 2 * kLayPf rows follow
        uint32_t cur[kLayPf], nxt[kLayPf];
        float bc[kLayPf], bn[kLayPf], pc[kLayPf], pn[kLayPf], ac[kLayPf], an[kLayPf], qc[kLayPf], qn[kLayPf];
#pragma unroll
        for (int k = 0; k < kLayPf; ++k) {
            cur[k] = plan[(size_t)k * LW];
            bc[k] = bet[(size_t)k * LW];
            pc[k] = betp[(size_t)k * LW];
            ac[k] = OA ? oma[(size_t)k * LW] : 0.0f;
            qc[k] = OA ? omap[(size_t)k * LW] : 0.0f;
        }
        for (int i0 = 0; i0 < m; i0 += kLayPf) {
#pragma unroll
            for (int k = 0; k < kLayPf; ++k) {
                const size_t e = (size_t)(i0 + kLayPf + k) * LW;
                nxt[k] = plan[e];
                bn[k] = bet[e];
                pn[k] = betp[e];
                an[k] = OA ? oma[e] : 0.0f;
                qn[k] = OA ? omap[e] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < kLayPf; ++k) step(cur[k], bc[k], pc[k], ac[k], qc[k], i0 + k);
#pragma unroll
            for (int k = 0; k < kLayPf; ++k) { cur[k] = nxt[k]; bc[k] = bn[k]; pc[k] = pn[k]; ac[k] = an[k]; qc[k] = qn[k]; }
        }
        if (ES) {
            const unsigned unsat = syndrome();
            if (frozen == 0u && unsat == 0u) { frozen = 1u; my_iters = it + 1; }
        }
    }
    asm volatile("" ::: "memory");

    unsigned ok;
    if (ES) ok = (row_live && frozen != 0u) ? 1u : 0u;
    else ok = syndrome() == 0u ? 1u : 0u;
    if (row_live && row < cw && t == 0) {
        if (iterations) iterations[b0 + row] = (ES && ok) ? my_iters : T;
        if (success) success[b0 + row] = (uint8_t)ok;
    }
    const int nbytes = (n + 7) / 8;
    for (int r = 0; r < cw; ++r) {
        if (b0 + r >= batch) break;
        const size_t ob = (size_t)(b0 + r) * n;
        for (int j0 = 0; j0 < n; j0 += kWave) {
            const int j = j0 + lane;
            const bool in = j < n;
            const float v = in ? lay_lds_ld((unsigned)r * row_bytes + (unsigned)j * 4u) : 0.0f;
            const bool neg = in && v < 0.0f;
            if (in && posterior) __builtin_nontemporal_store(v, posterior + ob + j);
            if (in && bits) __builtin_nontemporal_store(neg ? 1 : 0, bits + ob + j);
            if (packed) {
                const unsigned long long mk = __ballot(neg);
                if (lane < 8 && j0 + 8 * lane < n) packed[(size_t)(b0 + r) * nbytes + (j0 >> 3) + lane] = (uint8_t)(mk >> (8 * lane));
            }
        }
    }
}

// beta_lay[it][entry] = beta[it][slot[entry]] (1 where slot < 0): the paper kernel's beta, in plan order
__global__ void lay_beta_gather(const float *__restrict__ beta, int n_beta, const int *__restrict__ slot, int entries, int T,
                                float *__restrict__ out)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (long long)entries * T) return;
    const int it = (int)(k / entries), s = slot[k % entries];
    out[k] = s >= 0 ? beta[(size_t)it * n_beta + s] : 1.0f;
}

}  // namespace ldpc
