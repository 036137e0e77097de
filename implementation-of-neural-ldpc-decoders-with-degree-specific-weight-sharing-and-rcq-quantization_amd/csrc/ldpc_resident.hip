// ldpc_resident.hip -- LDS-resident fused decoder (gfx950): all T iterations of G codewords
// run inside ONE workgroup with every message in LDS; HBM sees only the LLRs in and the
// decisions out (~16 KB per codeword instead of T*(16E+4n) ~ 1.15 MB for the (1998,1512) code).
//
// Mapping (the transpose of the streaming kernels): lanes run over the NODES of the graph,
// the G codewords of the workgroup ride along as a G-wide vector per lane (ds_read/write_b64
// for G = 2, b128 for G = 4).
//   msg  [S][G]  fp32   at LDS offset 0; one slot per edge, "ELL-transposed" check-major:
//                       slot(p,t) = t*m + p  (p = position of the check after sorting by degree)
//                       -> consecutive lanes hit consecutive LDS words in the check phase
//   llr_s[n][G]  fp32   channel LLRs in degree-sorted variable order
//   bits_s[n]    u8     hard decisions of the G codewords (bit g), for the syndrome
//   alpha_s      fp32   the [T][n_alpha] V2C weight table (when it is small)
// One array holds both message directions in place: the check phase turns v2c into c2v slot by
// slot, the variable phase gathers its dv slots (byte offsets, 8 x u16 in one 16-byte load), forms
// the leave-one-out sums in the reference's association order and scatters v2c back.
//
// The engine is bound by instruction issue, not by LDS or HBM, so the phases are written for
// instruction count: nodes are sorted by degree and every wave whose lanes share one degree (all
// but the class-boundary waves) runs wave-uniform control flow -- scalar loop counters, one scalar
// branch into the compile-time body of its degree; min1/min2 by v_med3; the sign product as an XOR
// of raw bit patterns; index lists fetched one variable ahead.
// Arithmetic is the streaming kernels' (same helpers), so the two engines give identical results
// (the GPU parity tests run every case on both).
//
// Early stop (reference semantics): every iteration a posterior pass + syndrome pass finds the
// codewords that just converged; their posterior is recomputed into their (now dead) LLR slots
// and written out at once; the workgroup leaves when all G are done.
#pragma once

#include "ldpc_kernels.hip"
#include "ldpc_resident_geom.h"

namespace ldpc {

struct ResidentPlan {
    int n, m, S, max_dc, max_dv;
    int mstride;                  // slots between consecutive edges of a check: slot(p,t) = t*mstride + p
                                  // (512 when m <= 512 so that LDS instructions can carry t*stride as an
                                  //  immediate offset; else m)
    const uint8_t *dc_s;          // [m]          degree of the (sub-)check at sorted position p
    const uint8_t *gsz;           // [m] or null  lane-group size of position p: a check wider than the slot layout admits is
                                  //              split over 2^k ADJACENT lanes (sub-checks of contiguous edges); 1 = whole check
    int any_split;                // some check is split (gsz != null): the host launches the SPLIT instantiation of the kernel
    int par_words;                // m when the row stride is a power of two: parity words of the early-stop syndrome (ParScatter)
    int par_shift;                // log2 of the bytes per slot
    const uint16_t *cvar;         // [max_dc*m]   sorted position of the variable of edge (p,t)
    const uint16_t *bslot;        // [max_dc*m]   beta table column of edge (p,t)
    const uint16_t *bslot_c;      // [m] or null: column shared by all edges of check p (Basic, RCQ,
                                  //              sharing types 2-4) -> one table read per check
    const uint16_t *oaslot;       // [max_dc*m]   OMS alpha column (or null)
    const uint32_t *vmeta;        // [n]          degree | alpha column << 8 of sorted variable q
    const uint2 *vslot_lo;        // [n]          LDS byte offsets (= slot * G * 4, all <= 65535) of edges k = 0..3 of q, four
                                  //              16-bit values in 8 bytes
    const uint2 *vslot_hi;        // [n_hi]       ... of edges k = 4..7, for the n_hi leading (highest-degree) variables only
    int n_hi;                     //              variables of degree > 4 (they come first in the degree-sorted order)
                                  // 8 + 8 + 4 bytes per variable: the whole plan of the (1998,1512) code is 26 KB and stays in
                                  // the CU's 32 KiB L1 across iterations (with 32-bit offsets and the hi half read for every
                                  // variable it was 72 KB per workgroup and iteration from L2)
    const uint16_t *inv_perm_v;   // [n]          sorted position of original variable j
    int n_pos;                    //              positions in use: n, or (compact plan) the highest occupied one + 1
    unsigned vcell[8];            // compact plan: byte r of word w = the cell (wave w, round r) -- kCell* below
    unsigned ccell[8];            // compact plan: word w = the checks of wave w (positions 64w .. 64w+63) -- kChk* below
    int E;                        // edges of the graph
    const uint32_t *edge_of_slot; // [S]          CSR edge id held by a slot, 0xffffffff for padding slots (test hook
                                  //              ldpc_debug_resident_c2v: dumps the C2V state in CSR order)
};

struct ResidentArgs {
    const float *llr;             // [batch][n]
    long long batch;
    int T, early_stop;
    const float *beta; int n_beta;
    const float *alpha; int n_alpha;
    const float *oms_alpha; int n_oms_alpha;
    const float *thr; int n_levels; const int *q_of_iter;
    int *bits; float *posterior; int *iterations; uint8_t *success; uint8_t *packed;
    int alpha_in_lds;             // T * n_alpha floats staged in LDS
    int unit_alpha;               // every alpha == 1.0f (Basic, RCQ, sharing types 1/3): the multiply is skipped
    int rcq_zero0;                // every quantiser has tau_0 == 0 (true for gamma > 0): per-check quantisation
    void *dbg_c2v;                // [batch][E] or null: C2V values of every codeword's last executed iteration, CSR edge
                                  // order (include/ldpc_hip_debug.h; lets the tests compare per-edge RCQ codes on this engine)
};

// LDS access by byte offset.  The dynamic LDS block is this kernel's only LDS object (no static
// __shared__), so it starts at LDS address 0 and a message slot's byte offset IS its LDS address:
// addressing through an address-space-3 pointer built from the offset avoids the "+ base" VALU add
// that the generic-pointer form leaves on every access.  resident_decode traps if a static LDS
// allocation ever appears in front of the dynamic block.
template <typename X>
__device__ __forceinline__ X lds_load(unsigned byte_off)
{
    constexpr int N = sizeof(X) / sizeof(float);
    typedef float VT __attribute__((ext_vector_type(N)));
    using LP = __attribute__((address_space(3))) const VT *;
    union { VT v; X k; } u;
    u.v = *(LP)(size_t)byte_off;
    return u.k;
}
template <typename X>
__device__ __forceinline__ void lds_store(unsigned byte_off, const X &v)
{
    constexpr int N = sizeof(X) / sizeof(float);
    typedef float VT __attribute__((ext_vector_type(N)));
    using LP = __attribute__((address_space(3))) VT *;
    union { VT v; X k; } u;
    u.k = v;
    *(LP)(size_t)byte_off = u.v;
}

// LLRs in and decisions out are touched once per codeword: non-temporal, so that they do not evict the plan (the index data
// every iteration re-reads) from the CU's L1
template <typename X>
__device__ __forceinline__ X res_stream_load(const X *p) { return __builtin_nontemporal_load(p); }
template <typename X>
__device__ __forceinline__ void res_stream_store(X *p, X v) { __builtin_nontemporal_store(v, p); }

__device__ __forceinline__ void lds_atomic_xor(unsigned byte_off, unsigned v)
{
    using LP = __attribute__((address_space(3))) unsigned *;
    __hip_atomic_fetch_xor((LP)(size_t)byte_off, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Early-stop syndrome without a second gather: the variable lane that has just formed a hard decision XORs it into the
// parity word of each of its checks (one LDS atomic per edge).  The check position is recovered from the edge's slot
// offset -- slot(p,t) = t*stride + p with a power-of-two stride: p = (offset >> shift) & mask -- so no index data is
// loaded; `par_off` = 0 switches the scatter off (then the checks gather the decisions, res_syndrome_phase).
struct ParScatter {
    unsigned par_off = 0, shift = 0, mask = 0;
};

__device__ __forceinline__ bool wave_uniform(int v, int &vw)
{
    vw = __builtin_amdgcn_readfirstlane(v);
    return __ballot(v != vw) == 0ull;
}

// ---- check phase: v2c -> c2v in place, lane = check -----------------------------------------
//   pass 1  per value: min1' = med3(a, min1, -inf) = min, min2' = med3(a, min1, min2), signs ^= bits(x)
//   pass 2  re-reads the slot (LDS reads are cheap here): the arg-min edge is recognised by
//           |x| == min1 -- on a tie min2 == min1, so which tied edge "is" the arg-min is
//           value-irrelevant, exactly as with the reference's first-index argmin -- and the sign of
//           the product of the OTHER signs is bit 31 of (signs ^ x).
// quantise-and-reconstruct magnitude: tau[last q with mag >= tau_q], default tau_0; the q = 0
// comparison can never change the outcome and is left out (any threshold order, NaN included)
template <int NL>
__device__ __forceinline__ float res_quant_rec(float mag, const float (&th)[8], const float *__restrict__ thr, int n_levels)
{
    float rec = (n_levels <= 8) ? th[0] : thr[0];
    if constexpr (NL > 0) {                                   // compile-time level count (bc = 3: 4)
#pragma unroll
        for (int q = 1; q < NL; ++q) rec = (mag >= th[q]) ? th[q] : rec;
    } else if (n_levels <= 8) {
#pragma unroll
        for (int q = 1; q < 8; ++q) rec = (mag >= th[q]) ? th[q] : rec;   // NaN padding never matches
    } else {
        for (int q = 1; q < n_levels; ++q) rec = (mag >= thr[q]) ? thr[q] : rec;
    }
    return rec;
}

// ---- wide checks: one check split over a group of 2^k adjacent lanes ---------------------------------------------
// Each lane reduces its own edges (min1 / min2 / sign bits / zero count); the partials are combined across the group by
// an XOR butterfly of wavefront exchanges -- ds_swizzle (bit-mask mode, no LDS memory touched) inside 32 lanes, a
// cross-half shuffle for the last step -- after which every lane of the group holds the whole check's values and emits
// its own edges.  Steps beyond a lane's own group size are exchanged too (the instruction is wave-wide) but not combined.
template <int O>
__device__ __forceinline__ unsigned lane_xchg(unsigned v)
{
    if constexpr (O < 32) return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, (O << 10) | 0x1f);
    else return (unsigned)__shfl_xor((int)v, 32, 64);
}
template <int O> __device__ __forceinline__ float lane_xchg(float v) { return __uint_as_float(lane_xchg<O>(__float_as_uint(v))); }
template <int O>
__device__ __forceinline__ double lane_xchg(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = lane_xchg<O>((unsigned)u), hi = lane_xchg<O>((unsigned)(u >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

template <int O, int G, typename T>
__device__ __forceinline__ void group_step(int gs, T (&m1)[G], T (&m2)[G], unsigned (&sg)[G], unsigned (&nz)[G])
{
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const T a1 = lane_xchg<O>(m1[g]), a2 = lane_xchg<O>(m2[g]);
        const unsigned as = lane_xchg<O>(sg[g]), an = lane_xchg<O>(nz[g]);
        if (O < gs) {
            // second smallest of {m1, m2, a1, a2} = min(max(m1, a1), min(m2, a2)); ties keep min2 == min1
            const T hi = m1[g] < a1 ? a1 : m1[g];
            const T lo2 = m2[g] < a2 ? m2[g] : a2;
            m2[g] = hi < lo2 ? hi : lo2;
            m1[g] = m1[g] < a1 ? m1[g] : a1;
            sg[g] ^= as;
            nz[g] += an;
        }
    }
}
template <int G, typename T>
__device__ __forceinline__ void group_combine(int gs, T (&m1)[G], T (&m2)[G], unsigned (&sg)[G], unsigned (&nz)[G])
{
    group_step<1, G, T>(gs, m1, m2, sg, nz);
    group_step<2, G, T>(gs, m1, m2, sg, nz);
    group_step<4, G, T>(gs, m1, m2, sg, nz);
    group_step<8, G, T>(gs, m1, m2, sg, nz);
    group_step<16, G, T>(gs, m1, m2, sg, nz);
    group_step<32, G, T>(gs, m1, m2, sg, nz);
}
// parity words of the syndrome phases
__device__ __forceinline__ unsigned group_xor(int gs, unsigned x)
{
    unsigned y;
    y = lane_xchg<1>(x);  if (1 < gs) x ^= y;
    y = lane_xchg<2>(x);  if (2 < gs) x ^= y;
    y = lane_xchg<4>(x);  if (4 < gs) x ^= y;
    y = lane_xchg<8>(x);  if (8 < gs) x ^= y;
    y = lane_xchg<16>(x); if (16 < gs) x ^= y;
    y = lane_xchg<32>(x); if (32 < gs) x ^= y;
    return x;
}

// Pass 2 of the check phase for TWO edges of a codeword pair (four values), hand-scheduled: out = (|x| == min1 ? o2 : o1) ^
// sign(x).  Written in C the compiler emits compare -> s_nop -> v_cndmask per value (a lane mask needs two instructions
// between its compare and its reader) and keeps the sign-bit constant in an SGPR -- a v_bitop3_b32 with an SGPR operand
// issues in ~4.2 cycles instead of ~2.3 (tools/probes/valu_issue_probe.hip).  Four compares into four lane masks, four
// selects, four bitop3 with the constant in a VGPR: no padding, 10.7 instead of ~15.5 issue cycles per value.
__device__ __forceinline__ void res_select4(float &x0, float &x1, float &x2, float &x3, float m1a, float m1b,
                                            uint32_t o1a, uint32_t o2a, uint32_t o1b, uint32_t o2b, uint32_t sign_v)
{
    unsigned long long c0, c1, c2;
    uint32_t t0, t1, t2, t3;
    asm("v_cmp_eq_f32_e64 %8, |%0|, %11\n\t"
        "v_cmp_eq_f32_e64 %9, |%1|, %12\n\t"
        "v_cmp_eq_f32_e64 %10, |%2|, %11\n\t"
        "v_cmp_eq_f32_e64 vcc, |%3|, %12\n\t"
        "v_cndmask_b32_e64 %4, %13, %14, %8\n\t"
        "v_cndmask_b32_e64 %5, %15, %16, %9\n\t"
        "v_cndmask_b32_e64 %6, %13, %14, %10\n\t"
        "v_cndmask_b32_e32 %7, %15, %16, vcc\n\t"
        "v_bitop3_b32 %0, %4, %0, %17 bitop3:0x78\n\t"
        "v_bitop3_b32 %1, %5, %1, %17 bitop3:0x78\n\t"
        "v_bitop3_b32 %2, %6, %2, %17 bitop3:0x78\n\t"
        "v_bitop3_b32 %3, %7, %3, %17 bitop3:0x78"
        : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&s"(c0), "=&s"(c1), "=&s"(c2)
        : "v"(m1a), "v"(m1b), "v"(o1a), "v"(o2a), "v"(o1b), "v"(o2b), "v"(sign_v)
        : "vcc");
}

// res_select4 with the results in registers of their own.  An asm statement's in/out ("+v") operands are tied pairs, and
// the compiler copies a tied operand past the sixteenth into a scratch register and back (v_mov, s_nop, v_mov per
// call); with plain inputs and early-clobber outputs, which double as the selects' temporaries, nothing is copied.
__device__ __forceinline__ void res_select4_out(float (&y)[4], float x0, float x1, float x2, float x3, float m1a, float m1b,
                                                uint32_t o1a, uint32_t o2a, uint32_t o1b, uint32_t o2b, uint32_t sign_v)
{
    unsigned long long c0, c1, c2;
    asm("v_cmp_eq_f32_e64 %4, |%7|, %11\n\t"
        "v_cmp_eq_f32_e64 %5, |%8|, %12\n\t"
        "v_cmp_eq_f32_e64 %6, |%9|, %11\n\t"
        "v_cmp_eq_f32_e64 vcc, |%10|, %12\n\t"
        "v_cndmask_b32_e64 %0, %13, %14, %4\n\t"
        "v_cndmask_b32_e64 %1, %15, %16, %5\n\t"
        "v_cndmask_b32_e64 %2, %13, %14, %6\n\t"
        "v_cndmask_b32_e32 %3, %15, %16, vcc\n\t"
        "v_bitop3_b32 %0, %0, %7, %17 bitop3:0x78\n\t"
        "v_bitop3_b32 %1, %1, %8, %17 bitop3:0x78\n\t"
        "v_bitop3_b32 %2, %2, %9, %17 bitop3:0x78\n\t"
        "v_bitop3_b32 %3, %3, %10, %17 bitop3:0x78"
        : "=&v"(y[0]), "=&v"(y[1]), "=&v"(y[2]), "=&v"(y[3]), "=&s"(c0), "=&s"(c1), "=&s"(c2)
        : "v"(x0), "v"(x1), "v"(x2), "v"(x3), "v"(m1a), "v"(m1b), "v"(o1a), "v"(o2a), "v"(o1b), "v"(o2b), "v"(sign_v)
        : "vcc");
}

// Pass 1 of the check phase: the running two smallest magnitudes (m1 <= m2) of a check's inputs.
// One value at a time: m2' = med3(a, m1, m2), m1' = med3(a, m1, -inf) = min(a, m1) as ONE v_med3 (`ninf` is -inf in a
// register the optimiser cannot see through: a literal -inf is folded into canonicalise + v_min, three instructions).
__device__ __forceinline__ void res_min2_step(float &m1, float &m2, float x, float ninf)
{
    const float a = __builtin_fabsf(x);
    m2 = __builtin_amdgcn_fmed3f(a, m1, m2);
    m1 = __builtin_amdgcn_fmed3f(a, m1, ninf);
}
// Two values a, b of TWO codewords at a time: the two smallest of {m1, m2, a, b} are min3(m1, a, b) and
// min(m2, med3(m1, a, b)) -- the second smallest is m2 or the middle one of the other three, whichever is smaller.
// Three instructions of the slow class per two values instead of four, and the same bits for every input without a
// NaN: the two smallest elements of a multiset do not depend on how they are found (a magnitude has no -0).
// Written as asm because fminf in C gets a canonicalising v_max in front of it under IEEE mode.
__device__ __forceinline__ void res_min2_pair2(float &m1a, float &m2a, float &m1b, float &m2b, float xa0, float xa1,
                                               float xb0, float xb1)
{
    float ta, tb;
    asm("v_med3_f32 %4, %0, |%6|, |%8|\n\t"
        "v_med3_f32 %5, %2, |%7|, |%9|\n\t"
        "v_min3_f32 %0, %0, |%6|, |%8|\n\t"
        "v_min3_f32 %2, %2, |%7|, |%9|\n\t"
        "v_min_f32_e32 %1, %1, %4\n\t"
        "v_min_f32_e32 %3, %3, %5"
        : "+v"(m1a), "+v"(m2a), "+v"(m1b), "+v"(m2b), "=&v"(ta), "=&v"(tb)
        : "v"(xa0), "v"(xa1), "v"(xb0), "v"(xb1));
}
// the same for one codeword (the fp32 kernels with one codeword per workgroup, G == 1)
__device__ __forceinline__ void res_min2_pair(float &m1, float &m2, float xa, float xb)
{
    float t;
    asm("v_med3_f32 %2, %0, |%3|, |%4|\n\t"
        "v_min3_f32 %0, %0, |%3|, |%4|\n\t"
        "v_min_f32_e32 %1, %1, %2"
        : "+v"(m1), "+v"(m2), "=&v"(t)
        : "v"(xa), "v"(xb));
}
// sign accumulator over two values: ONE v_bitop3_b32 (a ^ b ^ c = 0x96) instead of two v_xor_b32
__device__ __forceinline__ uint32_t res_xor3(uint32_t acc, float xa, float xb)
{
    return __builtin_amdgcn_bitop3_b32(acc, __float_as_uint(xa), __float_as_uint(xb), 0x96);
}
// Two edges (xa, xb: the slots of the codeword pair) into the running state of G codewords.  FORM_RCQ keeps the one-value
// chain for the magnitudes: DESIGN.md 4 defines its NaN behaviour, which rests on v_med3's NaN rule; the parity is the
// same bits in either form.
template <int FORM, int G>
__device__ __forceinline__ void res_absorb2(float (&m1)[G], float (&m2)[G], uint32_t (&sacc)[G], const Pack<float, G> &xa,
                                            const Pack<float, G> &xb, float ninf)
{
#pragma unroll
    for (int g = 0; g < G; ++g) sacc[g] = res_xor3(sacc[g], xa.x[g], xb.x[g]);
    if constexpr (FORM == FORM_RCQ) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            res_min2_step(m1[g], m2[g], xa.x[g], ninf);
            res_min2_step(m1[g], m2[g], xb.x[g], ninf);
        }
    } else if constexpr (G == 2) {
        res_min2_pair2(m1[0], m2[0], m1[1], m2[1], xa.x[0], xa.x[1], xb.x[0], xb.x[1]);
    } else {
#pragma unroll
        for (int g = 0; g < G; ++g) res_min2_pair(m1[g], m2[g], xa.x[g], xb.x[g]);
    }
}

// test hook (ldpc_debug_min2): both forms of pass 1 on rows of d arbitrary values, two rows per thread as the two
// codewords of a pair -- the one-value chain with a two-input xor, and the edges in pairs with an odd last one through
// the one-value step (the walk of res_check_body_uniform and res_check_body).  No degree-1 rule is applied.
__global__ void debug_min2(const float *__restrict__ vals, long long rows, int d, float *__restrict__ m12_chain,
                           uint32_t *__restrict__ par_chain, float *__restrict__ m12_pair, uint32_t *__restrict__ par_pair)
{
    using P = Pack<float, 2>;
    const long long r0 = 2 * ((long long)blockIdx.x * blockDim.x + threadIdx.x);
    if (r0 >= rows) return;
    const bool two = r0 + 1 < rows;
    const float *ra = vals + r0 * d, *rb = vals + (two ? r0 + 1 : r0) * d;
    float ninf = -inf_of<float>();
    asm volatile("" : "+v"(ninf));
    float c1[2], c2[2], p1[2], p2[2];
    uint32_t cs[2], ps[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        c1[g] = c2[g] = p1[g] = p2[g] = inf_of<float>();
        cs[g] = ps[g] = 0;
    }
    for (int t = 0; t < d; ++t) {
        const P v{{ra[t], rb[t]}};
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            cs[g] ^= __float_as_uint(v.x[g]);
            res_min2_step(c1[g], c2[g], v.x[g], ninf);
        }
    }
    int t = 0;
    for (; t + 1 < d; t += 2) res_absorb2<FORM_NMS, 2>(p1, p2, ps, P{{ra[t], rb[t]}}, P{{ra[t + 1], rb[t + 1]}}, ninf);
    if (t < d) {
        const P v{{ra[t], rb[t]}};
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            ps[g] ^= __float_as_uint(v.x[g]);
            res_min2_step(p1[g], p2[g], v.x[g], ninf);
        }
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        if (g == 1 && !two) break;
        m12_chain[2 * (r0 + g)] = c1[g]; m12_chain[2 * (r0 + g) + 1] = c2[g]; par_chain[r0 + g] = cs[g];
        m12_pair[2 * (r0 + g)] = p1[g];  m12_pair[2 * (r0 + g) + 1] = p2[g];  par_pair[r0 + g] = ps[g];
    }
}

// the same for FOUR edges of one float64 codeword: compares on the 64-bit values, selects and sign on the 32-bit halves
__device__ __forceinline__ void res_select4_f64(double (&x)[4], double m1, double o1, double o2, uint32_t sign_v)
{
    const unsigned long long b1 = (unsigned long long)__double_as_longlong(o1), b2 = (unsigned long long)__double_as_longlong(o2);
    const uint32_t o1l = (uint32_t)b1, o1h = (uint32_t)(b1 >> 32), o2l = (uint32_t)b2, o2h = (uint32_t)(b2 >> 32);
    uint32_t xh[4], rl[4], rh[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xh[i] = (uint32_t)((unsigned long long)__double_as_longlong(x[i]) >> 32);
    unsigned long long c0, c1, c2;
    asm("v_cmp_eq_f64_e64 %[c0], |%[x0]|, %[m1]\n\t"
        "v_cmp_eq_f64_e64 %[c1], |%[x1]|, %[m1]\n\t"
        "v_cmp_eq_f64_e64 %[c2], |%[x2]|, %[m1]\n\t"
        "v_cmp_eq_f64_e64 vcc, |%[x3]|, %[m1]\n\t"
        "v_cndmask_b32_e64 %[l0], %[o1l], %[o2l], %[c0]\n\t"
        "v_cndmask_b32_e64 %[h0], %[o1h], %[o2h], %[c0]\n\t"
        "v_cndmask_b32_e64 %[l1], %[o1l], %[o2l], %[c1]\n\t"
        "v_cndmask_b32_e64 %[h1], %[o1h], %[o2h], %[c1]\n\t"
        "v_cndmask_b32_e64 %[l2], %[o1l], %[o2l], %[c2]\n\t"
        "v_cndmask_b32_e64 %[h2], %[o1h], %[o2h], %[c2]\n\t"
        "v_cndmask_b32_e32 %[l3], %[o1l], %[o2l], vcc\n\t"
        "v_cndmask_b32_e32 %[h3], %[o1h], %[o2h], vcc\n\t"
        "v_bitop3_b32 %[h0], %[h0], %[xh0], %[k] bitop3:0x78\n\t"
        "v_bitop3_b32 %[h1], %[h1], %[xh1], %[k] bitop3:0x78\n\t"
        "v_bitop3_b32 %[h2], %[h2], %[xh2], %[k] bitop3:0x78\n\t"
        "v_bitop3_b32 %[h3], %[h3], %[xh3], %[k] bitop3:0x78"
        : [l0] "=&v"(rl[0]), [h0] "=&v"(rh[0]), [l1] "=&v"(rl[1]), [h1] "=&v"(rh[1]), [l2] "=&v"(rl[2]), [h2] "=&v"(rh[2]),
          [l3] "=&v"(rl[3]), [h3] "=&v"(rh[3]), [c0] "=&s"(c0), [c1] "=&s"(c1), [c2] "=&s"(c2)
        : [x0] "v"(x[0]), [x1] "v"(x[1]), [x2] "v"(x[2]), [x3] "v"(x[3]), [m1] "v"(m1), [o1l] "v"(o1l), [o1h] "v"(o1h),
          [o2l] "v"(o2l), [o2h] "v"(o2h), [xh0] "v"(xh[0]), [xh1] "v"(xh[1]), [xh2] "v"(xh[2]), [xh3] "v"(xh[3]), [k] "v"(sign_v)
        : "vcc");
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = __longlong_as_double((long long)(((unsigned long long)rh[i] << 32) | rl[i]));
}

// Edges 0 .. dc-1 of a lane's check in ascending order with the loop control on the scalar unit: d_lo (wave-uniform) edges
// as groups of four plus a tail of two and of one on scalar branches, f(address of the group's first slot, edges in the
// group as a compile-time constant) -- the slots of a group sit at immediate offsets k*stride from one address register
// -- and then, only in a wave that holds several degrees, the lanes with dc > d_lo take their remaining edges one at a
// time under the exec mask.  A wave of one degree executes no exec-mask instruction and no per-trip vector compare.
template <typename F>
__device__ __forceinline__ void res_walk_edges(unsigned base, unsigned stride, int d_lo, int spread, int dc, F &&f)
{
    unsigned addr = base;
#pragma unroll 1
    for (int t = 0; t + 4 <= d_lo; t += 4) {
        f(addr, std::integral_constant<int, 4>{});
        addr += 4 * stride;
    }
    if (d_lo & 2) {
        f(addr, std::integral_constant<int, 2>{});
        addr += 2 * stride;
    }
    if (d_lo & 1) f(addr, std::integral_constant<int, 1>{});
#pragma unroll 1
    for (int e = d_lo; e < d_lo + spread; ++e)
        if (e < dc) f(base + (unsigned)e * stride, std::integral_constant<int, 1>{});
}

// How res_check_body_uniform walks a check's d_lo edges, a compile-time choice per instantiation like res_cpt_forms:
// 0 is res_walk_edges in both passes (groups of four, every edge read twice).  kChkHold: the last 4 + (d_lo & 3) edges
// are read as ONE group at the end of pass 1 and stay in registers, pass 2 starts with them -- select and write, no
// read, no wait -- and reads only the edges in front of them; kChkBy8 walks those in groups of eight (a group of four
// for the rest).  Degree 14 is [8][6] then [6 held][8]: three LDS round trips and 22 reads per phase instead of eight
// and 28.  An instantiation takes a part only where it stays within the 80 VGPRs of six waves per SIMD with no more
// scratch than without it (profiles/check_hold_compiler_report.txt).  With this compiler all three kernels of the
// select form do (72, 79 and 74 VGPRs, no scratch); the table is where one that stops doing so goes back to 0.
constexpr unsigned kChkHold = 1u;
constexpr unsigned kChkBy8 = 2u;
constexpr unsigned res_cpt_check_walk(int form, int nl)
{
    (void)form; (void)nl;
    return kChkHold | kChkBy8;
}

// pass 1 on the K edges v[K0 .. K0+K-1] held in registers, in index order: pairs, an odd last one by the one-value step
template <int FORM, int K0, int K, int N>
__device__ __forceinline__ void res_absorb_held(float (&m1)[2], float (&m2)[2], uint32_t (&sacc)[2],
                                                const Pack<float, 2> (&v)[N], float ninf)
{
    static_assert(K0 + K <= N, "edges of the array");
#pragma unroll
    for (int k = K0; k + 1 < K0 + K; k += 2) res_absorb2<FORM, 2>(m1, m2, sacc, v[k], v[k + 1], ninf);
    if constexpr (K & 1) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            sacc[g] ^= __float_as_uint(v[K0 + K - 1].x[g]);
            res_min2_step(m1[g], m2[g], v[K0 + K - 1].x[g], ninf);
        }
    }
}
// pass 2 on the same: edge k goes to addr + k * STRIDE.  An odd last edge is paired with itself, the copy's result dropped.
template <unsigned STRIDE, int K0, int K, int N>
__device__ __forceinline__ void res_select_held(unsigned addr, const Pack<float, 2> (&v)[N], const float (&m1)[2],
                                                const uint32_t (&o1)[2], const uint32_t (&o2)[2], uint32_t sign_v)
{
    static_assert(K0 + K <= N, "edges of the array");
#pragma unroll
    for (int k = K0; k < K0 + K; k += 2) {
        constexpr int last = K0 + K - 1;
        const int k1 = k + 1 <= last ? k + 1 : k;
        float y[4];
        res_select4_out(y, v[k].x[0], v[k].x[1], v[k1].x[0], v[k1].x[1], m1[0], m1[1], o1[0], o2[0], o1[1], o2[1], sign_v);
        lds_store<Pack<float, 2>>(addr + k * STRIDE, Pack<float, 2>{{y[0], y[1]}});
        if (k1 != k) lds_store<Pack<float, 2>>(addr + k1 * STRIDE, Pack<float, 2>{{y[2], y[3]}});
    }
}

// The check phase of the compact kernels (fp32 codeword pairs, no split checks) for a wave with d_lo >= 4, in the
// one-beta-per-check form (normalised min-sum, RCQ with tau_0 == 0): the two passes of res_check_body below -- the same
// arithmetic on the same edges in the same order, so every output is the same bits -- walked by res_walk_edges or,
// with WALK != 0, with the check's tail held between the passes (res_cpt_check_walk).  The
// host marks every wave of a decoder with per-edge tables or other forms kChkPerLane.
template <int FORM, int NL, int MS, unsigned WALK>
__device__ __forceinline__ void res_check_body_uniform(int p, int dc, unsigned cw, float b_check, const float (&th)[8],
                                                       const float *__restrict__ thr, int n_levels)
{
    static_assert(FORM == FORM_NMS || FORM == FORM_RCQ, "forms with two outgoing magnitudes per check");
    static_assert(MS > 0, "compile-time row stride: the slots of a group are immediate offsets");
    static_assert(WALK == 0 || (WALK & kChkHold), "groups of eight come with the held tail");
    constexpr int G = 2;
    using P = Pack<float, G>;
    constexpr unsigned stride = (unsigned)MS * G * (unsigned)sizeof(float);
    static_assert(7 * stride < 65536u, "immediate offsets of a group of eight");
    const unsigned base = (unsigned)p * G * (unsigned)sizeof(float);
    const int d_lo = chk_lo(cw), spread = chk_spread(cw);
    float m1[G], m2[G];
    uint32_t sacc[G];
    float ninf = -inf_of<float>();
    asm volatile("" : "+v"(ninf));                    // see res_check_body
#pragma unroll
    for (int g = 0; g < G; ++g) {
        m1[g] = inf_of<float>(); m2[g] = inf_of<float>(); sacc[g] = 0;
    }
    // the edges in front of the held tail: d_lo - 4 - (d_lo & 3) of them, a multiple of four, in groups of KB and one
    // group of four; f as in res_walk_edges
    constexpr int KB = (WALK & kChkBy8) ? 8 : 4;
    const int rem = d_lo & 3, body = d_lo - 4 - rem;
    auto walk_body = [&](auto &&f) -> unsigned {
        unsigned addr = base;
#pragma unroll 1
        for (int t = 0; t + KB <= body; t += KB) {
            f(addr, std::integral_constant<int, KB>{});
            addr += KB * stride;
        }
        if constexpr (KB == 8) {
            if (body & 4) {
                f(addr, std::integral_constant<int, 4>{});
                addr += 4 * stride;
            }
        }
        return addr;
    };
    // the lanes of a mixed-degree wave with dc > d_lo: their remaining edges one at a time under the exec mask
    auto walk_spread = [&](auto &&f) {
#pragma unroll 1
        for (int e = d_lo; e < d_lo + spread; ++e)
            if (e < dc) f(base + (unsigned)e * stride, std::integral_constant<int, 1>{});
    };
    auto pass1 = [&](unsigned addr, auto kc) {
        constexpr int K = decltype(kc)::value;
        P v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = lds_load<P>(addr + k * stride);
        res_absorb_held<FORM, 0, K>(m1, m2, sacc, v, ninf);
    };
    P tl[7];                                          // the held tail: edges body .. d_lo-1, tl[4 ..] as far as rem says
    unsigned ta = 0;
    if constexpr (WALK != 0) {
        ta = walk_body(pass1);
#pragma unroll
        for (int k = 0; k < 4; ++k) tl[k] = lds_load<P>(ta + k * stride);
        if (rem == 0) {
            res_absorb_held<FORM, 0, 4>(m1, m2, sacc, tl, ninf);
        } else if (rem == 1) {
            tl[4] = lds_load<P>(ta + 4 * stride);
            res_absorb_held<FORM, 0, 5>(m1, m2, sacc, tl, ninf);
        } else if (rem == 2) {
            tl[4] = lds_load<P>(ta + 4 * stride);
            tl[5] = lds_load<P>(ta + 5 * stride);
            res_absorb_held<FORM, 0, 6>(m1, m2, sacc, tl, ninf);
        } else {
            tl[4] = lds_load<P>(ta + 4 * stride);
            tl[5] = lds_load<P>(ta + 5 * stride);
            tl[6] = lds_load<P>(ta + 6 * stride);
            res_absorb_held<FORM, 0, 7>(m1, m2, sacc, tl, ninf);
        }
        walk_spread(pass1);
    }
    if constexpr (WALK == 0)
    res_walk_edges(base, stride, d_lo, spread, dc, [&](unsigned addr, auto kc) {
        constexpr int K = decltype(kc)::value;
        P v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = lds_load<P>(addr + k * stride);
        // the edges of a group in pairs (res_absorb2); a group of one -- the odd tail, and each spread edge of a
        // mixed-degree wave -- takes the one-value step
        if constexpr (K == 1) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                sacc[g] ^= __float_as_uint(v[0].x[g]);
                res_min2_step(m1[g], m2[g], v[0].x[g], ninf);
            }
        } else {
#pragma unroll
            for (int k = 0; k < K; k += 2) res_absorb2<FORM, G>(m1, m2, sacc, v[k], v[k + 1], ninf);
        }
    });

    uint32_t o1[G], o2[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float w1 = b_check * m1[g], w2 = b_check * m2[g];
        if (FORM == FORM_RCQ) {
            const float r1 = res_quant_rec<NL>(__builtin_fabsf(w1), th, thr, n_levels);
            const float r2 = res_quant_rec<NL>(__builtin_fabsf(w2), th, thr, n_levels);
            w1 = flip_sign<float>(r1, (w1 < 0.0f) ? 1u : 0u);
            w2 = flip_sign<float>(r2, (w2 < 0.0f) ? 1u : 0u);
        }
        const uint32_t par = sacc[g] & 0x80000000u;
        o1[g] = __float_as_uint(w1) ^ par;
        o2[g] = __float_as_uint(w2) ^ par;
        asm volatile("" : "+v"(o1[g]), "+v"(o2[g]));
    }
    uint32_t sign_v = 0x80000000u;
    asm volatile("" : "+v"(sign_v));
    if constexpr (WALK != 0) {
        // the held tail first -- nothing to wait for -- then the edges in front of it, read again
        res_select_held<stride, 0, 4>(ta, tl, m1, o1, o2, sign_v);
        if (rem == 1) res_select_held<stride, 4, 1>(ta, tl, m1, o1, o2, sign_v);
        else if (rem == 2) res_select_held<stride, 4, 2>(ta, tl, m1, o1, o2, sign_v);
        else if (rem == 3) res_select_held<stride, 4, 3>(ta, tl, m1, o1, o2, sign_v);
        auto pass2 = [&](unsigned addr, auto kc) {
            constexpr int K = decltype(kc)::value;
            P v[K];
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = lds_load<P>(addr + k * stride);
            res_select_held<stride, 0, K>(addr, v, m1, o1, o2, sign_v);
        };
        walk_body(pass2);
        walk_spread(pass2);
        return;
    }
    // every edge goes through res_select4_out (the constant in a VGPR); an odd edge is paired with a dummy pair whose
    // result is dropped
    res_walk_edges(base, stride, d_lo, spread, dc, [&](unsigned addr, auto kc) {
        constexpr int K = decltype(kc)::value;
        P v[4];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = lds_load<P>(addr + k * stride);
        if constexpr (K & 1) asm volatile("" : "=v"(v[K].x[0]), "=v"(v[K].x[1]));    // any two registers
#pragma unroll
        for (int k = 0; k < K; k += 2) {
            float y[4];
            res_select4_out(y, v[k].x[0], v[k].x[1], v[k + 1].x[0], v[k + 1].x[1], m1[0], m1[1], o1[0], o2[0], o1[1], o2[1],
                            sign_v);
            lds_store<P>(addr + k * stride, P{{y[0], y[1]}});
            if (k + 1 < K) lds_store<P>(addr + (k + 1) * stride, P{{y[2], y[3]}});
        }
    });
}

// PAIRS = false keeps pass 1 one edge at a time: the compact OMS kernels, which spill more with the pair form
template <int G, int FORM, bool BPC, int NL, int MS, typename T, bool SPLIT = false, bool PAIRS = true>
__device__ __forceinline__ void res_check_body(const ResidentPlan &pl, unsigned char *smem, int p, int dc,
                                               T b_check, const T *__restrict__ beta_row,
                                               const T *__restrict__ oa_row, const float (&th)[8],
                                               const float *__restrict__ thr, int n_levels, bool rcq_zero0, int gs = 1)
{
    // Per-lane degrees; with SPLIT the lanes of a group (gs > 1) hold the pieces of ONE wide check: their partials are
    // combined between the two passes.
    constexpr int kEl = G * (int)sizeof(T);
    const int trip = dc;
    const unsigned stride = (MS > 0 ? (unsigned)MS : (unsigned)pl.mstride) * kEl;   // compile-time when MS > 0
    const unsigned base = (unsigned)p * kEl;
    if constexpr (!std::is_same<T, float>::value) {
        // fp64 (BasicMinSumDecoder with the reference's own float64 LLRs): normalised min-sum with one factor per
        // check, the same two passes in plain compare/select form (v_med3 / v_bitop3 are 32-bit instructions)
        static_assert(FORM == FORM_NMS && BPC, "the fp64 resident engine covers the per-check normalised form");
        using PD = Pack<T, G>;
        T m1[G], m2[G];
        unsigned par[G];
#pragma unroll
        for (int g = 0; g < G; ++g) { m1[g] = inf_of<T>(); m2[g] = inf_of<T>(); par[g] = 0; }
        auto absorb = [&](const PD &v) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                par[g] ^= signbit_of<T>(v.x[g]);
                // "if a < min1: (min2, min1) = (min1, a) elif a < min2: min2 = a" (ldpc_decoder.py:96-101) without branches:
                // min2' = max(min(a, min2), min1), min1' = min(a, min1) -- the same values for every ordered input, and a NaN
                // is skipped by both forms (v_min/v_max_f64 return the other operand for a quiet NaN; the initial pass
                // quiets the caller's LLRs, arithmetic never produces a signalling one).  Three instructions instead of two
                // compares, two exec-mask branches and five 64-bit moves.
                T lo, m1n;
                asm("v_min_f64 %0, |%1|, %2" : "=v"(lo) : "v"(v.x[g]), "v"(m2[g]));
                asm("v_min_f64 %0, |%1|, %2" : "=v"(m1n) : "v"(v.x[g]), "v"(m1[g]));
                asm("v_max_f64 %0, %1, %2" : "=v"(m2[g]) : "v"(lo), "v"(m1[g]));
                m1[g] = m1n;
            }
        };
        {
            int t = 0;
            for (; t + 3 < trip; t += 4) {
                const unsigned addr = base + t * stride;
                const PD va = lds_load<PD>(addr), vb = lds_load<PD>(addr + stride);
                const PD vc = lds_load<PD>(addr + 2 * stride), vd = lds_load<PD>(addr + 3 * stride);
                absorb(va); absorb(vb); absorb(vc); absorb(vd);
            }
            for (; t < trip; ++t) absorb(lds_load<PD>(base + t * stride));
        }
        if constexpr (SPLIT) {
            unsigned nzd[G];
#pragma unroll
            for (int g = 0; g < G; ++g) nzd[g] = 0;
            group_combine<G, T>(gs, m1, m2, par, nzd);
        }
        T o1[G], o2[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (trip == 1 && gs == 1) m2[g] = m1[g];        // "min2_val = min_val" for a degree-1 check
            o1[g] = flip_sign<T>(b_check * m1[g], par[g]);
            o2[g] = flip_sign<T>(b_check * m2[g], par[g]);
            asm volatile("" : "+v"(o1[g]), "+v"(o2[g]));   // two products per check, not one v_mul_f64 per edge (see the fp32 form)
        }
        int t = 0;
        if constexpr (G == 1) {
            uint32_t sign_v = 0x80000000u;
            asm volatile("" : "+v"(sign_v));
            for (; t + 3 < trip; t += 4) {
                const unsigned addr = base + t * stride;
                T x[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] = lds_load<PD>(addr + i * stride).x[0];
                res_select4_f64(x, m1[0], o1[0], o2[0], sign_v);
#pragma unroll
                for (int i = 0; i < 4; ++i) { PD o; o.x[0] = x[i]; lds_store<PD>(addr + i * stride, o); }
            }
        }
#pragma unroll 4
        for (; t < trip; ++t) {
            const unsigned addr = base + t * stride;
            const PD v = lds_load<PD>(addr);
            PD o;
#pragma unroll
            for (int g = 0; g < G; ++g)
                o.x[g] = flip_sign<T>((abs_of<T>(v.x[g]) == m1[g]) ? o2[g] : o1[g], signbit_of<T>(v.x[g]));
            lds_store<PD>(addr, o);
        }
        return;
    } else {
    using P = Pack<float, G>;
    float m1[G], m2[G];
    uint32_t sacc[G];
    unsigned nz[G];
    float ninf = -inf_of<float>();
    asm volatile("" : "+v"(ninf));                    // opaque to constant folding (see below)
#pragma unroll
    for (int g = 0; g < G; ++g) {
        m1[g] = inf_of<float>(); m2[g] = inf_of<float>(); sacc[g] = 0; nz[g] = 0;
    }
    // generic form (any degree, per-lane trip counts, per-edge beta, OMS): pass 1 streams the slots, pass 2 re-reads them
    // the edges in pairs (res_absorb2), an odd last one through the one-value step.  One pair per trip: with two pairs (four
    // loads) in flight the compact RCQ kernels at four levels spilled one VGPR more than the parent's loop
    if constexpr (PAIRS) {
        int t = 0;
#pragma unroll 1
        for (; t + 1 < trip; t += 2) {
            const unsigned addr = base + t * stride;
            const P va = lds_load<P>(addr), vb = lds_load<P>(addr + stride);
            if (FORM == FORM_OMS) {
#pragma unroll
                for (int g = 0; g < G; ++g) nz[g] += ((va.x[g] == 0.0f) ? 1u : 0u) + ((vb.x[g] == 0.0f) ? 1u : 0u);
            }
            res_absorb2<FORM, G>(m1, m2, sacc, va, vb, ninf);
        }
        if (t < trip) {
            const P v = lds_load<P>(base + t * stride);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                sacc[g] ^= __float_as_uint(v.x[g]);
                if (FORM == FORM_OMS) nz[g] += (v.x[g] == 0.0f) ? 1u : 0u;
                res_min2_step(m1[g], m2[g], v.x[g], ninf);
            }
        }
    } else {
#pragma unroll 4
        for (int t = 0; t < trip; ++t) {
            const P v = lds_load<P>(base + t * stride);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                sacc[g] ^= __float_as_uint(v.x[g]);
                if (FORM == FORM_OMS) nz[g] += (__builtin_fabsf(v.x[g]) == 0.0f) ? 1u : 0u;
                res_min2_step(m1[g], m2[g], v.x[g], ninf);
            }
        }
    }
    if constexpr (SPLIT) group_combine<G, float>(gs, m1, m2, sacc, nz);
    if (trip == 1 && gs == 1) {
#pragma unroll
        for (int g = 0; g < G; ++g) m2[g] = m1[g];     // "min2_val = min_val" for a degree-1 check
    }

    if (BPC && (FORM == FORM_NMS || (FORM == FORM_RCQ && rcq_zero0))) {
        // One beta per check: only two outgoing magnitudes exist per codeword, so scaling (and for RCQ the
        // whole quantise-reconstruct) is done twice per check instead of once per edge.  Per edge remains:
        // pick by |x| == min1, then xor in the edge's own sign bit (the parity of all signs is pre-folded).
        uint32_t o1[G], o2[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float w1 = b_check * m1[g], w2 = b_check * m2[g];
            if (FORM == FORM_RCQ) {
                // value = (1 - 2*(w < 0)) * tau[level(|w|)]; with tau_0 == 0 a zero magnitude reconstructs to
                // +-0, so applying the edge sign afterwards is value-identical to the reference's order
                const float r1 = res_quant_rec<NL>(__builtin_fabsf(w1), th, thr, n_levels);
                const float r2 = res_quant_rec<NL>(__builtin_fabsf(w2), th, thr, n_levels);
                w1 = flip_sign<float>(r1, (w1 < 0.0f) ? 1u : 0u);
                w2 = flip_sign<float>(r2, (w2 < 0.0f) ? 1u : 0u);
            }
            const uint32_t par = sacc[g] & 0x80000000u;
            o1[g] = __float_as_uint(w1) ^ par;
            o2[g] = __float_as_uint(w2) ^ par;
            // keep the two per-check values materialised: without the barrier the optimiser sinks the
            // multiply (and the quantiser) back behind the per-edge select
            asm volatile("" : "+v"(o1[g]), "+v"(o2[g]));
        }
        int t = 0;
        if constexpr (G == 2) {
            uint32_t sign_v = 0x80000000u;
            asm volatile("" : "+v"(sign_v));              // the constant in a VGPR (see res_select4)
            for (; t + 3 < trip; t += 4) {
                const unsigned addr = base + t * stride;
                P va = lds_load<P>(addr), vb = lds_load<P>(addr + stride);
                P vc = lds_load<P>(addr + 2 * stride), vd = lds_load<P>(addr + 3 * stride);
                res_select4(va.x[0], va.x[1], vb.x[0], vb.x[1], m1[0], m1[1], o1[0], o2[0], o1[1], o2[1], sign_v);
                lds_store<P>(addr, va);
                lds_store<P>(addr + stride, vb);
                res_select4(vc.x[0], vc.x[1], vd.x[0], vd.x[1], m1[0], m1[1], o1[0], o2[0], o1[1], o2[1], sign_v);
                lds_store<P>(addr + 2 * stride, vc);
                lds_store<P>(addr + 3 * stride, vd);
            }
            if (t + 1 < trip) {
                const unsigned addr = base + t * stride;
                P va = lds_load<P>(addr), vb = lds_load<P>(addr + stride);
                res_select4(va.x[0], va.x[1], vb.x[0], vb.x[1], m1[0], m1[1], o1[0], o2[0], o1[1], o2[1], sign_v);
                lds_store<P>(addr, va);
                lds_store<P>(addr + stride, vb);
                t += 2;
            }
        }
#pragma unroll 1
        for (; t < trip; ++t) {
            const unsigned addr = base + t * stride;
            const P v = lds_load<P>(addr);
            P o;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const uint32_t sel = (__builtin_fabsf(v.x[g]) == m1[g]) ? o2[g] : o1[g];
                // sel ^ (x & sign bit) as ONE v_bitop3_b32 (truth table a ^ (b & c) = 0x78); written with & and ^ the
                // compiler emits v_and + v_xor here
                o.x[g] = __uint_as_float(__builtin_amdgcn_bitop3_b32(sel, __float_as_uint(v.x[g]), 0x80000000u, 0x78));
            }
            lds_store<P>(addr, o);
        }
        return;
    }

    int slot = p;
    const int sstride = MS > 0 ? MS : pl.mstride;
#pragma unroll 2
    for (int t = 0; t < trip; ++t) {
        const unsigned addr = base + t * stride;
        const float b = BPC ? b_check : beta_row[pl.bslot[slot]];
        float oa = 0.0f;
        if (FORM == FORM_OMS && oa_row) oa = oa_row[pl.oaslot[slot]];
        const P v = lds_load<P>(addr);
        P o;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float a = __builtin_fabsf(v.x[g]);
            const float raw = (a == m1[g]) ? m2[g] : m1[g];
            const uint32_t sflip = (__float_as_uint(v.x[g]) ^ sacc[g]) & 0x80000000u;
            if (FORM == FORM_NMS) {
                o.x[g] = __uint_as_float(__float_as_uint(b * raw) ^ sflip);
            } else if (FORM == FORM_OMS) {
                const unsigned ownz = (a == 0.0f) ? 1u : 0u;
                const bool nonzero = (nz[g] - ownz) == 0;
                const float d = raw - b;
                const float r = d > 0.0f ? d : 0.0f;
                const float val = r - oa;
                o.x[g] = nonzero ? __uint_as_float(__float_as_uint(val) ^ sflip) : 0.0f;
            } else {
                // quantise + reconstruct in one go: value = (1 - 2*sign_bit) * tau[level]
                const float w = __uint_as_float(__float_as_uint(b * raw) ^ sflip);
                const float rec = res_quant_rec<NL>(__builtin_fabsf(w), th, thr, n_levels);
                o.x[g] = flip_sign<float>(rec, (w < 0.0f) ? 1u : 0u);
            }
        }
        lds_store<P>(addr, o);
        slot += sstride;
    }
    }   // fp32
}

// `dc_pre` / `b_pre` are the first round's degree and per-check beta, fetched by the caller ahead of
// the barrier so their global-memory latency is off the critical path.
// CPT (compact kernels): `cw` is the wave's word of ResidentPlan::ccell, in an SGPR; the kernels of the one-beta-per-check
// select form run the scalar-counted body on it, everything else the per-lane form below.
template <int G, int FORM, bool BPC, int NL, int MS, typename T, bool SPLIT, bool CPT = false>
__device__ __forceinline__ void res_check_phase(const ResidentPlan &pl, unsigned char *smem,
                                                const T *__restrict__ beta_row,
                                                const T *__restrict__ oa_row,
                                                const float *__restrict__ thr, int n_levels, bool rcq_zero0,
                                                int dc_pre, T b_pre, int tid, int nt, unsigned cw = 0)
{
    float th[8];
    if (FORM == FORM_RCQ) {
#pragma unroll
        for (int q = 0; q < 8; ++q) th[q] = (q < n_levels) ? thr[q] : __builtin_nanf("");
    }
    if constexpr (CPT && BPC && (FORM == FORM_NMS || FORM == FORM_RCQ)) {
        static_assert(G == 2 && !SPLIT && std::is_same<T, float>::value, "compact: fp32 codeword pairs, whole checks");
        // opaque per phase: the conditions derived from the word and the lane masks derived from the degree are
        // recomputed where they are used instead of being held in SGPR pairs across the iteration loop
        asm volatile("" : "+s"(cw));
        asm volatile("" : "+v"(dc_pre), "+v"(b_pre));
        if (!(cw & kChkPerLane)) {
            // position tid is the lane's only check (m <= kResCptStride < the thread count) and the prefetched degree and
            // beta are all it needs.  A full wave runs with no lane mask at all, the last one is masked once for the whole
            // phase, a wave without checks leaves.
            const int lanes = chk_lanes(cw);
            constexpr unsigned WALK = res_cpt_check_walk(FORM, NL);
            if (lanes == 64) res_check_body_uniform<FORM, NL, MS, WALK>(tid, dc_pre, cw, b_pre, th, thr, n_levels);
            else if ((tid & 63) < lanes) res_check_body_uniform<FORM, NL, MS, WALK>(tid, dc_pre, cw, b_pre, th, thr, n_levels);
            return;
        }
        // per-lane waves of these kernels: the form below on the lane's one check
        if (tid < pl.m)
            res_check_body<G, FORM, BPC, NL, MS, T>(pl, smem, tid, dc_pre, b_pre, beta_row, oa_row, th, thr, n_levels, rcq_zero0);
        return;
    }
    int dc = dc_pre;
    T b_check = b_pre;
    for (int p = tid; p < pl.m; p += nt) {
        if (p != tid) {
            dc = pl.dc_s[p];
            b_check = BPC ? beta_row[pl.bslot_c[p]] : (T)0;
        }
        if constexpr (SPLIT) {
            // a wave holding lane groups runs the per-lane form for all its lanes at once: the group exchange between the
            // passes needs every lane of a group at the same point of the program
            const int gs = pl.gsz[p];
            if (__ballot(gs > 1) != 0ull) {
                res_check_body<G, FORM, BPC, NL, MS, T, true>(pl, smem, p, dc, b_check, beta_row, oa_row, th, thr, n_levels, rcq_zero0, gs);
                continue;
            }
        }
        // every lane runs the edge loops with ITS degree as trip count (exec-masked vector loops): one pass per wave
        // whatever the mix of degrees.  At two workgroups per CU it measured fastest against scalar per-degree forms
        // (DESIGN.md 3c table); at six waves per SIMD the loop control it spends in the vector unit counts, and the compact
        // kernels of the select form take res_check_body_uniform above instead.
        res_check_body<G, FORM, BPC, NL, MS, T, false, !(CPT && FORM == FORM_OMS)>(pl, smem, p, dc, b_check, beta_row, oa_row, th,
                                                                                   thr, n_levels, rcq_zero0);
    }
}

// ---- variable phase, lane = variable ----------------------------------------------------------
// MODE 0: v2c = llr + alpha * sum(others), scattered back in place
// MODE 2: the same with alpha == 1 everywhere (1.0f * x == x exactly, the multiply is skipped)
// MODE 1: posterior -> hard-decision byte bits_s[q]; components in `emask` also overwrite their
//         (dead) LLR slot with the posterior so the output pass can read it in original order
// MODE 4 / 6: MODE 0 / 2 plus the hard-decision byte from the same gathered values -- the early-stop
//         iteration of callers that do not ask for the posterior (one gather pass instead of two)
// MODE 9: MODE 8 with the posterior of the `emask` components kept in *lreg (compact kernels: no llr_s, the slots are
//         still being read by other lanes)
// `lreg`: the variable's LLR pair held in registers (ResVarState), or null to read it from llr_s
// The compact kernels run MODE 0 / 2 / 9 of this body from res_cpt_gather + res_cpt_scatter (offsets extracted from the
// packed plan words at their use): a change to the sums, their order or the v2c expression here is to be made there too
// (a mixed cell of the same kernels runs this body; tests/test_gpu_var_rounds.py compares every cell kind with the
// streaming engine bit for bit)
template <int G, int DV, int MODE, typename T>
__device__ __forceinline__ void res_var_body(unsigned char *smem, T *__restrict__ llr_s,
                                             uint8_t *__restrict__ bits_s, int q, const uint4 &slo, const uint4 &shi,
                                             T a, unsigned emask, const ParScatter &ps, Pack<T, G> *lreg)
{
    using P = Pack<T, G>;
    constexpr int ORD = std::is_same<T, float>::value ? 0 : 1;       // torch.sum fp32 order / np.sum fp64 order
    P *L = reinterpret_cast<P *>(llr_s);
    const unsigned off[8] = {slo.x, slo.y, slo.z, slo.w, shi.x, shi.y, shi.z, shi.w};
    P x[DV > 0 ? DV : 1];
#pragma unroll
    for (int k = 0; k < DV; ++k) x[k] = lds_load<P>(off[k]);
    P l = lreg ? *lreg : L[q];
    if constexpr (MODE == 0 || MODE == 2 || MODE == 4 || MODE == 6) {
        P out[DV > 0 ? DV : 1];
        auto v2c = [&](T llr, T sum) { return (MODE & 2) ? llr + sum : llr + a * sum; };
        unsigned byte = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            T xs[DV > 0 ? DV : 1];
#pragma unroll
            for (int k = 0; k < DV; ++k) xs[k] = x[k].x[g];
            if constexpr ((MODE & 4) != 0) byte |= ((l.x[g] + sum_ct<DV, -1, ORD, T>(xs)) < (T)0 ? 1u : 0u) << g;
            if constexpr (DV >= 1) out[0].x[g] = v2c(l.x[g], sum_ct<DV - 1, 0, ORD, T>(xs));
            if constexpr (DV >= 2) out[1].x[g] = v2c(l.x[g], sum_ct<DV - 1, 1, ORD, T>(xs));
            if constexpr (DV >= 3) out[2].x[g] = v2c(l.x[g], sum_ct<DV - 1, 2, ORD, T>(xs));
            if constexpr (DV >= 4) out[3].x[g] = v2c(l.x[g], sum_ct<DV - 1, 3, ORD, T>(xs));
            if constexpr (DV >= 5) out[4].x[g] = v2c(l.x[g], sum_ct<DV - 1, 4, ORD, T>(xs));
            if constexpr (DV >= 6) out[5].x[g] = v2c(l.x[g], sum_ct<DV - 1, 5, ORD, T>(xs));
            if constexpr (DV >= 7) out[6].x[g] = v2c(l.x[g], sum_ct<DV - 1, 6, ORD, T>(xs));
            if constexpr (DV >= 8) out[7].x[g] = v2c(l.x[g], sum_ct<DV - 1, 7, ORD, T>(xs));
        }
#pragma unroll
        for (int k = 0; k < DV; ++k) lds_store<P>(off[k], out[k]);
        if constexpr ((MODE & 4) != 0) {
            bits_s[q] = (uint8_t)byte;
            if (ps.par_off) {
#pragma unroll
                for (int k = 0; k < DV; ++k) lds_atomic_xor(ps.par_off + (((off[k] >> ps.shift) & ps.mask) << 2), byte);
            }
        }
    } else {
        unsigned byte = 0;
        bool store = false;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            T xs[DV > 0 ? DV : 1];
#pragma unroll
            for (int k = 0; k < DV; ++k) xs[k] = x[k].x[g];
            const T post = l.x[g] + sum_ct<DV, -1, ORD, T>(xs);
            byte |= (post < (T)0 ? 1u : 0u) << g;
            if ((emask >> g) & 1u) { l.x[g] = post; store = true; }
        }
        if constexpr (MODE == 8 || MODE == 9) {
            // last pass of a fixed-T decode: the c2v values in this variable's slots are dead once read above, so the
            // hard decisions go there (bit g = codeword g) and the final syndrome reads them back with consecutive
            // addresses per check (res_syndrome_slots) instead of gathering bytes through global index loads
#pragma unroll
            for (int k = 0; k < DV; ++k) lds_store<unsigned>(off[k], byte);
        } else {
            bits_s[q] = (uint8_t)byte;
            if (ps.par_off) {
#pragma unroll
                for (int k = 0; k < DV; ++k) lds_atomic_xor(ps.par_off + (((off[k] >> ps.shift) & ps.mask) << 2), byte);
            }
        }
        if (store) {
            if constexpr (MODE == 9) *lreg = l;
            else L[q] = l;
        }
    }
}

__device__ __forceinline__ uint4 plan_unpack(const uint2 &p)
{
    return make_uint4(p.x & 0xffffu, p.x >> 16, p.y & 0xffffu, p.y >> 16);
}

// DMAX: the largest degree the caller can meet (the compact plan's rounds 1-3 hold degree <= 4 only)
template <int G, int MODE, typename T, int DMAX = 8>
__device__ __forceinline__ void res_var_dispatch(unsigned char *smem, T *__restrict__ llr_s,
                                                 uint8_t *__restrict__ bits_s, int q, int dv, const uint4 &slo,
                                                 const uint4 &shi, T a, unsigned emask, const ParScatter &ps,
                                                 Pack<T, G> *lreg = nullptr)
{
#define LDPC_RV(D) \
    case D: if constexpr (D <= DMAX) res_var_body<G, D, MODE, T>(smem, llr_s, bits_s, q, slo, shi, a, emask, ps, lreg); break;
    switch (dv) {
        LDPC_RV(0) LDPC_RV(1) LDPC_RV(2) LDPC_RV(3) LDPC_RV(4) LDPC_RV(5) LDPC_RV(6) LDPC_RV(7) LDPC_RV(8)
    default: break;   // host admits only max_dv <= 8 to this engine
    }
#undef LDPC_RV
}

// Register-resident variable state (REG kernels, n <= kResRegVars * blockDim.x and n_hi <= blockDim.x): lane tid owns
// the sorted variables q = tid + r * nt, r < kResRegVars; their plan entries (degree | alpha column, packed slot offsets)
// and LLR pairs are loaded ONCE per launch and every variable phase runs from registers -- no plan loads and no llr_s
// read per iteration.  The rounds are unrolled (the array indices must be compile-time to stay in registers); a wave
// whose variables all lie past n leaves at a scalar branch.  Degree > 4 variables all sit in round 0, so only that
// round carries the upper offset half.
template <typename T, int G>
struct ResVarState {
    unsigned meta[kResRegVars];   // vmeta of the variable, 0 past n (not kept by the compact kernels)
    uint2 plo[kResRegVars];       // vslot_lo
    uint2 phi0;                   // vslot_hi of the round-0 variable (degree > 4), else 0
    Pack<T, G> l[kResRegVars];    // channel LLRs as the variable phase reads them (llr_s contents)
    unsigned cells;               // compact kernels: this wave's word of ResidentPlan::vcell (wave-uniform, SGPR)
};

// element `i` (32-bit index) of a uniform table: global_load / global_store ... v_off, s[base], no 64-bit vector add
template <typename X>
__device__ __forceinline__ const X *res_at(const X *base, unsigned i)
{
    return reinterpret_cast<const X *>(reinterpret_cast<const char *>(base) + (size_t)(i * (unsigned)sizeof(X)));
}
template <typename X>
__device__ __forceinline__ X *res_at(X *base, unsigned i)
{
    return reinterpret_cast<X *>(reinterpret_cast<char *>(base) + (size_t)(i * (unsigned)sizeof(X)));
}

// ---- compact variable phase ---------------------------------------------------------------------
// What lives across the iteration loop is the packed plan words and the LLR pairs, nothing else.  Everything a rare path
// needs is formed where it is used, behind something the compiler cannot see through, so that it is not hoisted out of
// the loop into registers of its own (the four vmeta lane addresses, the bslot_c one and the constants of the mixed
// cell's per-lane switch took 14 VGPRs that way, and one of the addresses was reloaded from scratch every iteration).

// Offset k of a variable (an LDS byte offset: one 16-bit half of a packed plan word), extracted at its use.  The
// instruction is written out: to the compiler the result is not loop-invariant, so the up to 20 unpacked offsets of a
// lane stay out of the loop's registers, and the packed word is only read -- redefining the packed words once per phase
// through an empty asm, as res_var_phase_reg does, cost a second copy of five of them and a v_mov each per iteration.
template <int K>
__device__ __forceinline__ unsigned plan_offset(const uint2 &lo, const uint2 &hi)
{
    const unsigned w = K < 2 ? lo.x : K < 4 ? lo.y : K < 6 ? hi.x : hi.y;
    unsigned o;
    if constexpr ((K & 1) == 0) asm volatile("v_and_b32_e32 %0, 0xffff, %1" : "=v"(o) : "v"(w));
    else asm volatile("v_lshrrev_b32_e32 %0, 16, %1" : "=v"(o) : "v"(w));
    return o;
}

// an empty lane of a cell with holes (vslot_lo.y == kResHole; 0xffff is no variable's offset: they are multiples of 8).
// Tested on the extracted half, so that the compare stays in the loop too
__device__ __forceinline__ bool plan_is_hole(const uint2 &lo) { return plan_offset<3>(lo, lo) == 0xffffu; }

// vmeta of the lane's round-R position, "scalar base + 32-bit lane offset" with an opaque offset.  Read by a mixed cell
// (degree) and by a decoder with alpha columns (MODE 0); never by Basic or RCQ on a code without mixed cells
template <int R>
__device__ __forceinline__ unsigned res_cpt_vmeta(const ResidentPlan &pl, int tid)
{
    unsigned q = (unsigned)tid + (unsigned)(R * kResCptThreads);
    asm volatile("" : "+v"(q));
    return *res_at(pl.vmeta, q);
}

// the gather half of a uniform cell's body: DV offsets extracted (kept for the stores), DV reads, nothing waits for them here
template <int G, int DV, int NX>
__device__ __forceinline__ void res_cpt_gather(const uint2 &lo, const uint2 &hi, unsigned (&off)[NX], Pack<float, G> (&x)[NX])
{
    using P = Pack<float, G>;
    static_assert(DV >= 1 && DV <= NX && NX <= 8, "degree");
#define LDPC_CPT_LD(K) \
    if constexpr (DV > K) { off[K] = plan_offset<K>(lo, hi); x[K] = lds_load<P>(off[K]); }
    LDPC_CPT_LD(0) LDPC_CPT_LD(1) LDPC_CPT_LD(2) LDPC_CPT_LD(3) LDPC_CPT_LD(4) LDPC_CPT_LD(5) LDPC_CPT_LD(6) LDPC_CPT_LD(7)
#undef LDPC_CPT_LD
}

// the other half: res_var_body's sums (same sum_ct expressions, same order) from the gathered values.  MODE 0 / 2: v2c
// back in place; MODE 9: the decisions into the variable's slots and the posterior of the `emask` codewords into `l`
template <int G, int DV, int MODE, int NX>
__device__ __forceinline__ void res_cpt_scatter(const unsigned (&off)[NX], const Pack<float, G> (&x)[NX],
                                                Pack<float, G> &l, float a, unsigned emask)
{
    using P = Pack<float, G>;
    static_assert(MODE == 0 || MODE == 2 || MODE == 9, "compact: fixed-T register-state modes");
    P out[DV];
    unsigned byte = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float xs[DV];
#pragma unroll
        for (int k = 0; k < DV; ++k) xs[k] = x[k].x[g];
        if constexpr (MODE == 9) {
            const float post = l.x[g] + sum_ct<DV, -1, 0, float>(xs);
            byte |= (post < 0.0f ? 1u : 0u) << g;
            if ((emask >> g) & 1u) l.x[g] = post;
        } else {
            auto v2c = [&](float llr, float sum) { return MODE == 2 ? llr + sum : llr + a * sum; };
            if constexpr (DV >= 1) out[0].x[g] = v2c(l.x[g], sum_ct<DV - 1, 0, 0, float>(xs));
            if constexpr (DV >= 2) out[1].x[g] = v2c(l.x[g], sum_ct<DV - 1, 1, 0, float>(xs));
            if constexpr (DV >= 3) out[2].x[g] = v2c(l.x[g], sum_ct<DV - 1, 2, 0, float>(xs));
            if constexpr (DV >= 4) out[3].x[g] = v2c(l.x[g], sum_ct<DV - 1, 3, 0, float>(xs));
            if constexpr (DV >= 5) out[4].x[g] = v2c(l.x[g], sum_ct<DV - 1, 4, 0, float>(xs));
            if constexpr (DV >= 6) out[5].x[g] = v2c(l.x[g], sum_ct<DV - 1, 5, 0, float>(xs));
            if constexpr (DV >= 7) out[6].x[g] = v2c(l.x[g], sum_ct<DV - 1, 6, 0, float>(xs));
            if constexpr (DV >= 8) out[7].x[g] = v2c(l.x[g], sum_ct<DV - 1, 7, 0, float>(xs));
        }
    }
#define LDPC_CPT_ST(K) \
    if constexpr (DV > K) { \
        if constexpr (MODE == 9) lds_store<unsigned>(off[K], byte); \
        else lds_store<P>(off[K], out[K]); \
    }
    LDPC_CPT_ST(0) LDPC_CPT_ST(1) LDPC_CPT_ST(2) LDPC_CPT_ST(3) LDPC_CPT_ST(4) LDPC_CPT_ST(5) LDPC_CPT_ST(6) LDPC_CPT_ST(7)
#undef LDPC_CPT_ST
}

// one round of the compact variable phase on the wave's scalar cell word: an empty cell is skipped, a uniform cell
// branches on its scalar degree straight into the body (rounds 1-3 hold degree <= 4 only), a cell with holes masks its
// empty lanes once, only a mixed cell runs the per-lane switch, its degrees from vmeta
template <int G, int MODE, typename T, int R>
__device__ __forceinline__ void res_var_round_cpt(const ResidentPlan &pl, unsigned char *smem, const T *__restrict__ alpha_glb,
                                                  unsigned emask, int tid, unsigned cells, ResVarState<T, G> &st)
{
    using P = Pack<T, G>;
    constexpr int DMAX = R == 0 ? 8 : 4;
    const unsigned cd = (cells >> (8 * R)) & 0xffu;
    if (cd == kCellEmpty) return;
    const uint2 lo = st.plo[R], hi = st.phi0;
    if (cd == kCellMixed) {
        const unsigned meta = res_cpt_vmeta<R>(pl, tid);
        int dv = (int)(meta & 0xffu);
        asm volatile("" : "+v"(dv));       // plain compares against inline constants (an SDWA byte compare keeps its constants in VGPRs)
        const uint4 slo = make_uint4(plan_offset<0>(lo, hi), plan_offset<1>(lo, hi), plan_offset<2>(lo, hi), plan_offset<3>(lo, hi));
        uint4 shi = make_uint4(0, 0, 0, 0);
        if constexpr (R == 0) shi = make_uint4(plan_offset<4>(lo, hi), plan_offset<5>(lo, hi), plan_offset<6>(lo, hi), plan_offset<7>(lo, hi));
        T a = (T)0;
        if (MODE == 0) a = alpha_glb[meta >> 8];
        res_var_dispatch<G, MODE, T, DMAX>(smem, nullptr, nullptr, tid + R * kResCptThreads, dv, slo, shi, a, emask, ParScatter{},
                                           &st.l[R]);
        return;
    }
    T a = (T)0;
    if (MODE == 0) a = alpha_glb[res_cpt_vmeta<R>(pl, tid) >> 8];
    if ((cd & kCellHoles) && plan_is_hole(lo)) return;               // the empty lanes of the cell
    P x[DMAX];
    unsigned off[DMAX];
#define LDPC_RVU(D) \
    case D: \
        if constexpr (D <= DMAX) { res_cpt_gather<G, D>(lo, hi, off, x); res_cpt_scatter<G, D, MODE>(off, x, st.l[R], a, emask); } \
        break;
    switch (cd & 0xfu) {                                           // wave-uniform: scalar compares and branches
        LDPC_RVU(1) LDPC_RVU(2) LDPC_RVU(3) LDPC_RVU(4) LDPC_RVU(5) LDPC_RVU(6) LDPC_RVU(7) LDPC_RVU(8)
    default: break;
    }
#undef LDPC_RVU
}

template <int G, int MODE, typename T>
__device__ __forceinline__ void res_var_phase_cpt(const ResidentPlan &pl, unsigned char *smem, const T *__restrict__ alpha_glb,
                                                  unsigned emask, int tid, ResVarState<T, G> &st)
{
    static_assert(kResRegVars == 4 && std::is_same<T, float>::value, "four rounds, fp32");
    // the wave's cell word, opaque once per phase: every test of a cell's kind or degree is a scalar compare and branch at its
    // place in the loop (hoisted, the tests became lane masks in SGPR pairs -- more than there are, spilled to VGPR lanes)
    unsigned cells = st.cells;
    asm volatile("" : "+s"(cells));
    res_var_round_cpt<G, MODE, T, 0>(pl, smem, alpha_glb, emask, tid, cells, st);
    res_var_round_cpt<G, MODE, T, 1>(pl, smem, alpha_glb, emask, tid, cells, st);
    res_var_round_cpt<G, MODE, T, 2>(pl, smem, alpha_glb, emask, tid, cells, st);
    res_var_round_cpt<G, MODE, T, 3>(pl, smem, alpha_glb, emask, tid, cells, st);
}

template <int G, int MODE, typename T>
__device__ __forceinline__ void res_var_phase_reg(const ResidentPlan &pl, unsigned char *smem,
                                                  T *__restrict__ llr_s, uint8_t *__restrict__ bits_s,
                                                  const T *__restrict__ alpha_lds,
                                                  const T *__restrict__ alpha_glb, unsigned emask,
                                                  int tid, int nt, ResVarState<T, G> &st, const ParScatter &ps)
{
    // the packed entries are unpacked at the point of use, as in the streaming loop: an opaque redefinition per phase
    // keeps the compiler from hoisting 8 unpacked offsets per variable out of the iteration loop (they would not fit
    // the register budget of four waves per SIMD)
#pragma unroll
    for (int r = 0; r < kResRegVars; ++r) asm volatile("" : "+v"(st.meta[r]), "+v"(st.plo[r].x), "+v"(st.plo[r].y));
    asm volatile("" : "+v"(st.phi0.x), "+v"(st.phi0.y));
#pragma unroll
    for (int r = 0; r < kResRegVars; ++r) {
        const int q = tid + r * nt;
        if (__builtin_amdgcn_readfirstlane(q - (tid & 63)) >= pl.n) break;   // the whole wave is past the end
        if (q < pl.n) {
            const unsigned meta = st.meta[r];
            const uint4 slo = plan_unpack(st.plo[r]), shi = r == 0 ? plan_unpack(st.phi0) : make_uint4(0, 0, 0, 0);
            T a = (T)0;
            if (MODE == 0 || MODE == 4) a = alpha_lds ? alpha_lds[meta >> 8] : alpha_glb[meta >> 8];
            res_var_dispatch<G, MODE, T>(smem, llr_s, bits_s, q, (int)(meta & 0xffu), slo, shi, a, emask, ps, &st.l[r]);
        }
    }
}

// Index data (degree, alpha column, the slot offsets) of the NEXT variable of a lane is fetched from
// global memory (L1/L2 resident, shared by every workgroup) while the current one is processed.
// (A two-register-set ping-pong that avoids the hand-over copies doubled the code and measured no faster.)
// REG: the register-resident form above instead.
template <int G, int MODE, typename T, bool REG, bool CPT = false>
__device__ __forceinline__ void res_var_phase(const ResidentPlan &pl, unsigned char *smem,
                                              T *__restrict__ llr_s, uint8_t *__restrict__ bits_s,
                                              const T *__restrict__ alpha_lds,
                                              const T *__restrict__ alpha_glb, unsigned emask,
                                              int tid, int nt, ResVarState<T, G> &st,
                                              const ParScatter ps = ParScatter{})
{
    if constexpr (CPT) {
        static_assert(REG && (MODE == 0 || MODE == 2 || MODE == 9), "compact: fixed-T register-state modes");
        res_var_phase_cpt<G, MODE, T>(pl, smem, alpha_glb, emask, tid, st);
        return;
    } else if constexpr (REG) {
        res_var_phase_reg<G, MODE, T>(pl, smem, llr_s, bits_s, alpha_lds, alpha_glb, emask, tid, nt, st, ps);
        return;
    }
    const int n = pl.n, n_hi = pl.n_hi;
    // Plan loads are UNCONDITIONAL with clamped indices (a lane past the end re-reads the last entry, a variable of degree <= 4
    // reads the last `hi` entry: same cache lines, values unused): with a fixed number of loads per round the compiler waits for
    // the CURRENT variable's entries with vmcnt(3) and leaves the next one's in flight -- behind `if (q < n_hi)` it could not
    // count them and drained the queue (vmcnt(0)) right after issuing the prefetch, every round.
    const int hi_last = (n_hi > 0 ? n_hi : 1) - 1;
    int q = tid;
    unsigned meta = 0;
    uint2 plo = make_uint2(0, 0), phi = make_uint2(0, 0);           // packed offsets, unpacked at the point of use
    if (q < n) {
        meta = pl.vmeta[q];
        plo = pl.vslot_lo[q];
        phi = pl.vslot_hi[min(q, hi_last)];
    }
    while (q < n) {
        const int qn = q + nt;
        unsigned metan;
        uint2 plon, phin;
        {
            // 32-bit byte offsets against the scalar base (global_load ... v_off, s[base]): one shift per load instead of a
            // sign extension and a 64-bit add each
            const unsigned qc = (unsigned)min(qn, n - 1), qh = min(qc, (unsigned)hi_last);
            metan = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(pl.vmeta) + (size_t)(qc << 2));
            plon = *reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(pl.vslot_lo) + (size_t)(qc << 3));
            phin = *reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(pl.vslot_hi) + (size_t)(qh << 3));
        }
        const int dv = (int)(meta & 0xffu);
        const uint4 slo = plan_unpack(plo), shi = plan_unpack(phi);
        T a = (T)0;                                                      // LDS copy of the table when small
        if (MODE == 0 || MODE == 4) a = alpha_lds ? alpha_lds[meta >> 8] : alpha_glb[meta >> 8];
        // every lane jumps to the compile-time body of ITS degree (exec-masked dispatch): one pass per wave whatever the mix
        res_var_dispatch<G, MODE, T>(smem, llr_s, bits_s, q, dv, slo, shi, a, emask, ps);
        q = qn; meta = metan; plo = plon; phi = phin;
    }
}

// H @ bits mod 2 per check from the hard-decision bytes; OR of all checks' parities -> *sh_unsat
template <int G, bool SPLIT>
__device__ __forceinline__ void res_syndrome_phase(const ResidentPlan &pl, const uint8_t *__restrict__ bits_s,
                                                   unsigned *sh_unsat, int tid, int nt)
{
    unsigned acc = 0;
    for (int p = tid; p < pl.m; p += nt) {
        const int dc = pl.dc_s[p];
        int dcw;
        unsigned x = 0;
        if (wave_uniform(dc, dcw)) {
#pragma unroll 8
            for (int t = 0; t < dcw; ++t) x ^= bits_s[pl.cvar[t * pl.mstride + p]];
        } else {
            for (int t = 0; t < dc; ++t) x ^= bits_s[pl.cvar[t * pl.mstride + p]];
        }
        if constexpr (SPLIT) x = group_xor(pl.gsz[p], x);   // a split check's parity is the XOR over its lane group
        acc |= x;
    }
    if (acc) atomicOr(sh_unsat, acc);
}

// syndrome from the parity words the variable lanes scattered into (ParScatter): OR of all checks' parities -> *sh_unsat,
// and the words are cleared for the next iteration
template <int G, bool SPLIT>
__device__ __forceinline__ void res_parity_reduce(const ResidentPlan &pl, unsigned par_off, unsigned *sh_unsat, int tid, int nt)
{
    unsigned acc = 0;
    for (int p = tid; p < pl.m; p += nt) {
        unsigned x = lds_load<unsigned>(par_off + 4u * (unsigned)p);
        lds_store<unsigned>(par_off + 4u * (unsigned)p, 0u);
        if constexpr (SPLIT) x = group_xor(pl.gsz[p], x);
        acc |= x;
    }
    if (acc) atomicOr(sh_unsat, acc);
}

// final syndrome of a fixed-T decode from the hard decisions res_var_body<MODE 8> left in the message slots
template <int G, typename T, bool SPLIT>
__device__ __forceinline__ void res_syndrome_slots(const ResidentPlan &pl, unsigned *sh_unsat, int tid, int nt)
{
    constexpr unsigned kSlot = sizeof(Pack<T, G>);
    unsigned acc = 0;
    for (int p = tid; p < pl.m; p += nt) {
        const int dc = pl.dc_s[p];
        int dcw;
        unsigned x = 0;
        if (wave_uniform(dc, dcw)) {
            // two slots per step: x ^ a ^ b is one v_bitop3_b32
            int t = 0;
#pragma unroll 4
            for (; t + 1 < dcw; t += 2)
                x = __builtin_amdgcn_bitop3_b32(x, lds_load<unsigned>((unsigned)(t * pl.mstride + p) * kSlot),
                                                lds_load<unsigned>((unsigned)((t + 1) * pl.mstride + p) * kSlot), 0x96);
            if (t < dcw) x ^= lds_load<unsigned>((unsigned)(t * pl.mstride + p) * kSlot);
        } else {
            for (int t = 0; t < dc; ++t) x ^= lds_load<unsigned>((unsigned)(t * pl.mstride + p) * kSlot);
        }
        if constexpr (SPLIT) x = group_xor(pl.gsz[p], x);
        acc |= x;
    }
    if (acc) atomicOr(sh_unsat, acc);
}

// ---- outputs ---------------------------------------------------------------------------------------------
// Positions are walked in ORIGINAL variable order j = tid + k*nt (coalesced row stores); the inverse-permutation
// entries of a batch of kEmit positions are loaded before the first LDS read (one round trip per batch), and the
// bit-packed row (the multi-GPU wire format) falls out of a wave ballot over 64 consecutive positions: lanes 0..7
// store the 8 bytes.  `mask`: codewords of the workgroup to write.
constexpr int kEmit = 4;

template <int G>
__device__ __forceinline__ void res_store_packed(const ResidentArgs &a, long long b, int j, int n, bool neg)
{
    const unsigned long long m = __ballot(neg);
    const int lane = threadIdx.x & 63;
    const int base = j - lane;                       // first position of this wave's 64
    if (lane < 8 && base + 8 * lane < n) a.packed[(size_t)b * ((n + 7) / 8) + (base >> 3) + lane] = (uint8_t)(m >> (8 * lane));
}

// posterior of the masked codewords sits in llr_s[.][g] (sorted order)
template <int G, typename T>
__device__ __forceinline__ void res_emit(const ResidentPlan &pl, const ResidentArgs &a, const T *__restrict__ llr_s,
                                         long long b0, unsigned mask, int iters, unsigned unsat, int tid, int nt)
{
    using P = Pack<T, G>;
    T *posterior = reinterpret_cast<T *>(a.posterior);
    const int n = pl.n;
    if (a.posterior || a.bits || a.packed) {
        for (int j0 = tid; j0 < n; j0 += kEmit * nt) {
            unsigned ip[kEmit];
#pragma unroll
            for (int k = 0; k < kEmit; ++k) ip[k] = (j0 + k * nt < n) ? pl.inv_perm_v[j0 + k * nt] : 0u;
#pragma unroll
            for (int k = 0; k < kEmit; ++k) {
                const int j = j0 + k * nt;
                if (j - (tid & 63) >= n) break;                       // the whole wave is past the row (wave-uniform)
                const bool in = j < n;
                const P p = reinterpret_cast<const P *>(llr_s)[ip[k]];  // ip = 0 for lanes past the row: harmless read
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (!((mask >> g) & 1u)) continue;
                    if (in && a.posterior) res_stream_store(&posterior[(size_t)(b0 + g) * n + j], p.x[g]);
                    if (in && a.bits) res_stream_store(&a.bits[(size_t)(b0 + g) * n + j], p.x[g] < (T)0 ? 1 : 0);
                    if (a.packed) res_store_packed<G>(a, b0 + g, j, n, in && p.x[g] < (T)0);
                }
            }
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (!((mask >> g) & 1u)) continue;
            if (a.iterations) a.iterations[b0 + g] = iters;
            if (a.success) a.success[b0 + g] = (uint8_t)(((unsat >> g) & 1u) ? 0 : 1);
        }
    }
}

// outputs when no posterior was asked for: hard decisions straight from bits_s (sorted order, bit g = codeword g)
template <int G>
__device__ __forceinline__ void res_emit_bits(const ResidentPlan &pl, const ResidentArgs &a, const uint8_t *__restrict__ bits_s,
                                              long long b0, unsigned mask, int iters, unsigned unsat, int tid, int nt)
{
    const int n = pl.n;
    if (a.bits || a.packed) {
        for (int j0 = tid; j0 < n; j0 += kEmit * nt) {
            unsigned ip[kEmit];
#pragma unroll
            for (int k = 0; k < kEmit; ++k) ip[k] = (j0 + k * nt < n) ? pl.inv_perm_v[j0 + k * nt] : 0u;
#pragma unroll
            for (int k = 0; k < kEmit; ++k) {
                const int j = j0 + k * nt;
                if (j - (tid & 63) >= n) break;
                const bool in = j < n;
                const unsigned bb = bits_s[ip[k]];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (!((mask >> g) & 1u)) continue;
                    const unsigned bit = (bb >> g) & 1u;
                    if (in && a.bits) res_stream_store(&a.bits[(size_t)(b0 + g) * n + j], (int)bit);
                    if (a.packed) res_store_packed<G>(a, b0 + g, j, n, in && bit != 0);
                }
            }
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (!((mask >> g) & 1u)) continue;
            if (a.iterations) a.iterations[b0 + g] = iters;
            if (a.success) a.success[b0 + g] = (uint8_t)(((unsat >> g) & 1u) ? 0 : 1);
        }
    }
}

// test hook: C2V values sitting in the message slots -> dbg_c2v[b][e] for the codewords in `mask`
template <int G, typename T>
__device__ __forceinline__ void res_dump_c2v(const ResidentPlan &pl, const ResidentArgs &a, long long b0, unsigned mask,
                                             int tid, int nt)
{
    using P = Pack<T, G>;
    T *out = reinterpret_cast<T *>(a.dbg_c2v);
    for (int s = tid; s < pl.S; s += nt) {
        const unsigned e = pl.edge_of_slot[s];
        if (e == 0xffffffffu) continue;
        const P v = lds_load<P>((unsigned)s * (unsigned)sizeof(P));
#pragma unroll
        for (int g = 0; g < G; ++g)
            if ((mask >> g) & 1u) out[(size_t)(b0 + g) * pl.E + e] = v.x[g];
    }
}

// ---- compact kernels: entry and exit of a full block ---------------------------------------------------------
// A compact plan has n <= n_pos <= kCptRows * kResCptThreads, so the rows of a codeword are ONE trip of kCptRows
// positions j = tid + k * kResCptThreads per lane.  The fast forms below serve a workgroup whose G codewords all exist
// (b0 + G <= batch, block-uniform) on a code with n > (kCptRows - 1) * kResCptThreads: rows 0 .. kCptRows-2 are full in
// every wave and carry no bound at all; the last row is decided per wave on the scalar unit (`jw` = the wave's first j).
// Everything else -- the padded last block, shorter codes -- keeps the per-element loops of the general kernels.
constexpr int kCptRows = 4;
// which of these forms an instantiation takes: the ones whose register allocation they cost scratch keep the general
// kernels' form of that part (profiles/r18_compiler_report.txt).  The table follows one compiler's spills, not the
// algorithm: compile the subsets again when the compiler changes (the report says how), and drop a fallback as soon as
// its instantiation takes the new part without more scratch -- each one is a second form of that part to maintain
constexpr unsigned kCptEntry = 1u;    // plan words ahead of the LLR loads, unbounded staging of a full block
constexpr unsigned kCptInit = 2u;     // init scatter on the scalar cell degree
constexpr unsigned kCptExit = 4u;     // syndrome walk, early inverse-permutation loads, specialised output pass
constexpr unsigned res_cpt_forms(int form, bool bpc, int nl)
{
    if (form == FORM_OMS) return bpc ? kCptEntry | kCptInit : kCptInit;      // the exit (and, per edge, the entry) spill
    if (form == FORM_RCQ && nl == 4 && !bpc) return kCptEntry | kCptInit;    // the exit spills
    return kCptEntry | kCptInit | kCptExit;
}
static_assert(kCptRows == kResRegVars, "the staging rows are the register rounds");

// a row pointer of the block (uniform), pinned to an SGPR pair: the address of an element stays "scalar base + 32-bit lane
// offset" instead of being re-associated into 64-bit vector adds shared between the rows.  The pin goes through an integer
// and comes back as a global-memory pointer (a pointer that passes through inline asm is a flat one to the compiler:
// flat_load / flat_store behind a 64-bit vector add each)
template <typename X>
__device__ __forceinline__ X *res_row(X *base, size_t elems)
{
    unsigned long long row = (unsigned long long)(base + elems);
    asm volatile("" : "+s"(row));
    return (X *)(__attribute__((address_space(1))) X *)row;
}

// the fast forms apply (block-uniform).  Opaque on purpose: evaluated at the entry and again at the exit
template <int G>
__device__ __forceinline__ bool res_cpt_full_block(const ResidentPlan &pl, const ResidentArgs &a, long long b0)
{
    int rows = kCptRows - 1;
    asm volatile("" : "+s"(rows));
    return b0 + G <= a.batch && pl.n > rows * kResCptThreads;
}

// The plan words of the entry, issued ahead of the LLR loads so that all of them return in one round trip: the wave's
// cell and check words (SGPRs), the lane's slot offsets of its four rounds, the degree of its check and its beta column.
// No load is conditional (one basic block): an empty cell reads the entries of cell 0, a lane past n_hi / past m the
// last entry -- values nothing uses (an empty cell is skipped everywhere, the upper offsets are read by degree > 4
// bodies only, the check phases mask lanes without a check).
template <int G, bool BPC>
__device__ __forceinline__ void res_cpt_plan_loads(const ResidentPlan &pl, int tid, unsigned wbase, ResVarState<float, G> &st,
                                                   unsigned &chk_cells, int &dc_pre, unsigned &bcol)
{
    const unsigned lane = (unsigned)tid - wbase;
    st.cells = pl.vcell[wbase >> 6];
    chk_cells = pl.ccell[wbase >> 6];
#pragma unroll
    for (int r = 0; r < kResRegVars; ++r) {
        const unsigned qb = ((st.cells >> (8 * r)) & 0xffu) ? wbase + (unsigned)(r * kResCptThreads) : 0u;   // scalar
        st.plo[r] = *res_at(pl.vslot_lo, qb + lane);               // padded to whole cells
    }
    st.phi0 = *res_at(pl.vslot_hi, min((unsigned)tid, (unsigned)max(pl.n_hi, 1) - 1u));
    const unsigned pc = min((unsigned)tid, (unsigned)pl.m - 1u);
    dc_pre = *res_at(pl.dc_s, pc);
    bcol = BPC ? *res_at(pl.bslot_c, pc) : 0u;
}

// LLR rows of a full block into the staging rows (sorted order), all loads before the first LDS store.  The partial
// wave of the last row clamps j: its lanes past the row load and store element n-1 once more (same value, same place).
template <int G>
__device__ __forceinline__ void res_cpt_stage_llrs(const ResidentPlan &pl, const float *__restrict__ g_llr, long long b0, int tid,
                                                   unsigned wbase)
{
    using P = Pack<float, G>;
    constexpr int K = kCptRows, NT = kResCptThreads;
    const unsigned n = (unsigned)pl.n;
    const float *row[G];
#pragma unroll
    for (int g = 0; g < G; ++g) row[g] = res_row(g_llr, (size_t)(b0 + g) * n);
    unsigned ip[K];
    P v[K];
#pragma unroll
    for (int k = 0; k < K - 1; ++k) {
        const unsigned j = (unsigned)tid + (unsigned)(k * NT);
        ip[k] = *res_at(pl.inv_perm_v, j);
#pragma unroll
        for (int g = 0; g < G; ++g) v[k].x[g] = res_stream_load(res_at(row[g], j));
    }
    const bool last = wbase + (unsigned)((K - 1) * NT) < n;         // wave-uniform: some lane of the last row is inside
    if (last) {
        const unsigned j = min((unsigned)tid + (unsigned)((K - 1) * NT), n - 1u);
        ip[K - 1] = *res_at(pl.inv_perm_v, j);
#pragma unroll
        for (int g = 0; g < G; ++g) v[K - 1].x[g] = res_stream_load(res_at(row[g], j));
    }
#pragma unroll
    for (int k = 0; k < K - 1; ++k) lds_store<P>(ip[k] * (unsigned)sizeof(P), v[k]);
    if (last) lds_store<P>(ip[K - 1] * (unsigned)sizeof(P), v[K - 1]);
}

// init scatter of round R on the wave's scalar cell degree (as res_var_round_cpt dispatches the phases): a uniform cell
// stores its dv times behind scalar branches, a cell with holes is masked once, only a mixed cell compares per lane and edge
template <int G, int R>
__device__ __forceinline__ void res_cpt_init_round(const ResidentPlan &pl, const ResVarState<float, G> &st, int tid, bool zero)
{
    using P = Pack<float, G>;
    const unsigned cd = (st.cells >> (8 * R)) & 0xffu;
    if (cd == kCellEmpty) return;
    const uint4 slo = plan_unpack(st.plo[R]), shi = R == 0 ? plan_unpack(st.phi0) : make_uint4(0, 0, 0, 0);
    const unsigned off[8] = {slo.x, slo.y, slo.z, slo.w, shi.x, shi.y, shi.z, shi.w};
    P l = st.l[R];
    if (zero) {                                                    // T == 0: c2v = 0
#pragma unroll
        for (int g = 0; g < G; ++g) l.x[g] = 0.0f;
    }
    if (cd == kCellMixed) {
        const int dv = (int)(pl.vmeta[tid + R * kResCptThreads] & 0xffu);
#pragma unroll
        for (int e = 0; e < (R == 0 ? 8 : 4); ++e)
            if (e < dv) lds_store<P>(off[e], l);
        return;
    }
    if ((cd & kCellHoles) && st.plo[R].y == kResHole) return;       // the empty lanes of the cell
    const int dv = (int)(cd & 0xfu);                               // wave-uniform: scalar compares and branches
#pragma unroll
    for (int e = 0; e < (R == 0 ? 8 : 4); ++e)
        if (e < dv) lds_store<P>(off[e], l);
}

// final syndrome of a compact decode: position tid is the lane's only check, its row of decisions sits at immediate
// offsets k * MS slots from one address; the walk is the check phase's (scalar trip counts from the wave's check word),
// four slots per group, pairs folded by the three-input xor
template <int G, int MS>
__device__ __forceinline__ void res_cpt_syndrome_slots(unsigned cw, int dc, unsigned *sh_unsat, int tid)
{
    constexpr unsigned kSlot = sizeof(Pack<float, G>), stride = (unsigned)MS * kSlot;
    auto body = [&]() {
        unsigned x = 0;
        res_walk_edges((unsigned)tid * kSlot, stride, chk_lo(cw), chk_spread(cw), dc, [&](unsigned addr, auto kc) {
            constexpr int K = decltype(kc)::value;
            unsigned v[K];
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = lds_load<unsigned>(addr + k * stride);
            if constexpr (K == 1) {
                x ^= v[0];
            } else {
#pragma unroll
                for (int k = 0; k < K; k += 2) x = __builtin_amdgcn_bitop3_b32(x, v[k], v[k + 1], 0x96);
            }
        });
        if (x) atomicOr(sh_unsat, x);
    };
    const int lanes = chk_lanes(cw);
    if (lanes == 64) body();
    else if ((tid & 63) < lanes) body();
}

// output pass of a full block: `ip` = the inverse-permutation entries of the lane's kCptRows positions (loaded by the
// caller ahead of the exit's barriers; the last row's j clamped as in res_cpt_stage_llrs), posteriors in the staging
// rows.  What was asked for is tested once per output, outside the rows; the last row's partial wave is masked once.
template <int G>
__device__ __forceinline__ void res_cpt_emit(const ResidentPlan &pl, const ResidentArgs &a, long long b0, const unsigned (&ip)[kCptRows],
                                             int iters, unsigned unsat, int tid, unsigned wbase)
{
    using P = Pack<float, G>;
    constexpr int K = kCptRows, NT = kResCptThreads;
    const unsigned n = (unsigned)pl.n, jl = (unsigned)tid + (unsigned)((K - 1) * NT), jwl = wbase + (unsigned)((K - 1) * NT);
    const bool last = jwl < n;                                      // wave-uniform, as in res_cpt_stage_llrs
    const bool part = jwl + 64u > n;                                // ... and only this wave of the last row is masked
    if (a.posterior || a.bits || a.packed) {
        P p[K];
#pragma unroll
        for (int k = 0; k < K - 1; ++k) p[k] = lds_load<P>(ip[k] * (unsigned)sizeof(P));
        if (last) p[K - 1] = lds_load<P>(ip[K - 1] * (unsigned)sizeof(P));
        if (a.posterior) {
            float *row[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                row[g] = res_row(a.posterior, (size_t)(b0 + g) * n);
#pragma unroll
                for (int k = 0; k < K - 1; ++k) res_stream_store(res_at(row[g], (unsigned)tid + (unsigned)(k * NT)), p[k].x[g]);
            }
            if (last && (!part || jl < n)) {
#pragma unroll
                for (int g = 0; g < G; ++g) res_stream_store(res_at(row[g], jl), p[K - 1].x[g]);
            }
        }
        if (a.bits) {
            int *row[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                row[g] = res_row(a.bits, (size_t)(b0 + g) * n);
#pragma unroll
                for (int k = 0; k < K - 1; ++k)
                    res_stream_store(res_at(row[g], (unsigned)tid + (unsigned)(k * NT)), p[k].x[g] < 0.0f ? 1 : 0);
            }
            if (last && (!part || jl < n)) {
#pragma unroll
                for (int g = 0; g < G; ++g) res_stream_store(res_at(row[g], jl), p[K - 1].x[g] < 0.0f ? 1 : 0);
            }
        }
        if (a.packed) {
            // a wave's 64 consecutive positions are 8 bytes of the row: ballot, lanes 0..7 store one byte each
            const unsigned lane = (unsigned)tid - wbase, nb = (n + 7u) >> 3;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                uint8_t *row = res_row(a.packed, (size_t)(b0 + g) * nb);
#pragma unroll
                for (int k = 0; k < K - 1; ++k) {
                    const unsigned long long m = __ballot(p[k].x[g] < 0.0f);
                    if (lane < 8) *res_at(row, ((wbase + (unsigned)(k * NT)) >> 3) + lane) = (uint8_t)(m >> (8 * lane));
                }
                if (last) {
                    const unsigned long long m = __ballot(jl < n && p[K - 1].x[g] < 0.0f);
                    if (lane < 8 && jwl + 8 * lane < n) *res_at(row, (jwl >> 3) + lane) = (uint8_t)(m >> (8 * lane));
                }
            }
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (a.iterations) a.iterations[b0 + g] = iters;
            if (a.success) a.success[b0 + g] = (uint8_t)(((unsat >> g) & 1u) ? 0 : 1);
        }
    }
}

// ES: 0 = fixed-iteration kernel, 1 = early-stop kernel (kept apart so that the fixed-T kernel does not carry
// the posterior/syndrome/emit code of the stop rule: the extra code cost the hot loop ~4 % when merged)
constexpr int kResMaxThreads = 1024;   // launch bounds of resident_decode: threads per workgroup, waves per SIMD the
constexpr int kResMinWaves = 4;        // register allocation must leave room for
// REG: variable state in registers (ResVarState; the host takes it for fixed-T decodes of codes that qualify, see
// resident_reg_state)
// CPT: compact fixed-T kernel (REG, fp32, no split checks): res_cpt_lds_total bytes of LDS, so that kResCptBlocks
// workgroups share a CU (build_resident_plan)
template <int G, int FORM, bool BPC, int NL, int MS, int ES, typename T = float, bool SPLIT = false, bool REG = false,
          bool CPT = false>
__global__ __launch_bounds__(CPT ? kResCptThreads : kResMaxThreads, CPT ? kResCptWaves : kResMinWaves)
void resident_decode(ResidentPlan pl, ResidentArgs a)
{
    static_assert(!CPT || (REG && !ES && !SPLIT && std::is_same<T, float>::value), "compact: fixed-T fp32 REG kernels only");
    extern __shared__ __align__(16) unsigned char res_smem[];     // the only LDS object: msg starts at offset 0
    if (__builtin_amdgcn_groupstaticsize() != 0) __builtin_trap();  // lds_load/lds_store rely on that (folds away)
    // T = float: G codewords per workgroup; T = double (fp64 Basic): the same 8-byte slots hold ONE codeword, so the
    // LDS carve is that of GE = G * sizeof(T) / 4 float codewords.  Table / LLR / posterior pointers of ResidentArgs are
    // typed float for the common case and re-read as T here.
    constexpr int GE = G * (int)(sizeof(T) / 4);
    const int n_alpha_lds = a.alpha_in_lds ? a.T * a.n_alpha * (int)(sizeof(T) / 4) : 0;
    // CPT: the LLR rows are staged at offset 0, in the message area the init scatter writes only after they are read
    T *llr_s = reinterpret_cast<T *>(res_smem + (CPT ? 0 : res_off_llr(pl.S, GE)));
    // CPT: no alpha table, decision bytes or parity words in the carve, and nothing that touches them is compiled
    T *alpha_s = CPT ? nullptr : reinterpret_cast<T *>(res_smem + res_off_alpha(pl.S, pl.n, GE));
    uint8_t *bits_s = CPT ? nullptr : res_smem + res_off_bits(pl.S, pl.n, GE, n_alpha_lds);
    unsigned *sh_unsat = reinterpret_cast<unsigned *>(res_smem + (CPT ? res_cpt_off_flag(pl.S, GE)
                                                                        : res_off_flag(pl.S, pl.n, GE, n_alpha_lds)));
    ParScatter ps, psf;                                  // per-iteration syndrome (early stop) / final syndrome (fixed T)
    if (!CPT && pl.par_words) {
        psf.par_off = (unsigned)res_off_par(pl.S, pl.n, GE, n_alpha_lds);
        psf.shift = (unsigned)pl.par_shift;
        psf.mask = (unsigned)pl.mstride - 1u;
        if (ES) ps = psf;
    }
    const T *g_llr = reinterpret_cast<const T *>(a.llr);
    const T *g_beta = reinterpret_cast<const T *>(a.beta);
    const T *g_alpha = reinterpret_cast<const T *>(a.alpha);
    const T *g_oms_alpha = reinterpret_cast<const T *>(a.oms_alpha);
    using P = Pack<T, G>;
    const int tid = threadIdx.x, nt = blockDim.x, n = pl.n;
    const long long b0 = (long long)blockIdx.x * G;
    constexpr unsigned kAll = (1u << G) - 1u;

    // LLRs: coalesced rows from HBM, scattered into degree-sorted order; padding codewords get +1.
    // All loads of a batch of kPro positions are issued before the first LDS store: one HBM round trip per
    // batch instead of one per element (the plain loop waits for every load before it issues the next).
    constexpr int kPro = 4;
    // compact kernels: the plan words first (res_cpt_plan_loads), then a full block of a code with a full third row
    // stages its rows without bounds (`cpt_fast`, block-uniform)
    ResVarState<T, G> st{};
    unsigned chk_cells = 0;                              // compact kernels: this wave's check word, in an SGPR
    int dc_cpt = 0;
    unsigned bcol_cpt = 0;
    bool cpt_fast = false;
    constexpr unsigned EE = CPT ? res_cpt_forms(FORM, BPC, NL) : 0u;
    if constexpr ((EE & kCptEntry) != 0) {
        const unsigned wbase = (unsigned)__builtin_amdgcn_readfirstlane(tid) & ~63u;
        res_cpt_plan_loads<G, BPC>(pl, tid, wbase, st, chk_cells, dc_cpt, bcol_cpt);
        cpt_fast = res_cpt_full_block<G>(pl, a, b0);
        if (cpt_fast) res_cpt_stage_llrs<G>(pl, g_llr, b0, tid, wbase);
    }
    for (int j0 = tid; j0 < (cpt_fast ? 0 : n); j0 += kPro * nt) {
        unsigned ip[kPro];
        P v[kPro];
#pragma unroll
        for (int k = 0; k < kPro; ++k) {
            const int j = j0 + k * nt;
            ip[k] = 0;
            if (j < n) {
                ip[k] = pl.inv_perm_v[j];
#pragma unroll
                for (int g = 0; g < G; ++g)
                    v[k].x[g] = (b0 + g < a.batch) ? res_stream_load(&g_llr[(size_t)(b0 + g) * n + j]) : (T)1;
            }
        }
#pragma unroll
        for (int k = 0; k < kPro; ++k)
            if (j0 + k * nt < n) reinterpret_cast<P *>(llr_s)[ip[k]] = v[k];
    }
    if constexpr (!CPT) {
        for (int k = tid; k < (a.alpha_in_lds ? a.T * a.n_alpha : 0); k += nt) alpha_s[k] = g_alpha[k];
    }
    if (tid == 0) { sh_unsat[0] = 0; sh_unsat[1] = 0; }
    if constexpr (!CPT) {
        for (int k = tid; k < pl.par_words; k += nt) lds_store<unsigned>(psf.par_off + 4u * (unsigned)k, 0u);
    }
    // first-round check degree (iteration-invariant) and per-check beta of iteration 0, in registers
    int dc_pre = 0;
    T b_pre = (T)0;
    if constexpr ((EE & kCptEntry) != 0) {
        // the beta of iteration 0 follows its column as soon as that is here: in flight across the barriers of the entry
        dc_pre = dc_cpt;
        if (BPC && a.T > 0) b_pre = *res_at(g_beta, bcol_cpt);
    }
    __syncthreads();
    // "initialise v2c with the channel LLRs" (T == 0: c2v = 0, the loop never runs)
    if constexpr (CPT) {
        // the lane's positions q = tid + r*nt of the host's grid: LLR pairs (and, in the kernels that do not load them at
        // the top, the plan entries) into registers once per launch, the wave's cell word into an SGPR
        if constexpr ((EE & kCptEntry) != 0) {
            // a position past n_pos reads the last staged row: nothing uses it
#pragma unroll
            for (int r = 0; r < kResRegVars; ++r)
                st.l[r] = lds_load<P>(min((unsigned)tid + (unsigned)(r * kResCptThreads), (unsigned)pl.n_pos - 1u) * (unsigned)sizeof(P));
        } else {
            // empty cells load nothing, empty lanes of a cell keep kResHole
            st.cells = pl.vcell[__builtin_amdgcn_readfirstlane(tid) >> 6];
            const P *L = reinterpret_cast<const P *>(llr_s);
#pragma unroll
            for (int r = 0; r < kResRegVars; ++r) {
                const int q = tid + r * nt;
                if (q < pl.n_pos) st.l[r] = L[q];                     // the staging rows hold positions < n_pos
                if ((st.cells >> (8 * r)) & 0xffu) {
                    st.plo[r] = pl.vslot_lo[q];                       // padded to whole cells
                    if (r == 0 && q < pl.n_hi) st.phi0 = pl.vslot_hi[q];
                }
            }
        }
        __syncthreads();                                   // the init scatter below overwrites the staged LLR rows
        if constexpr ((EE & kCptInit) != 0) {
            static_assert(kResRegVars == 4, "four rounds");
            res_cpt_init_round<G, 0>(pl, st, tid, a.T == 0);
            res_cpt_init_round<G, 1>(pl, st, tid, a.T == 0);
            res_cpt_init_round<G, 2>(pl, st, tid, a.T == 0);
            res_cpt_init_round<G, 3>(pl, st, tid, a.T == 0);
        } else {
#pragma unroll
            for (int r = 0; r < kResRegVars; ++r) {
                const unsigned cd = (st.cells >> (8 * r)) & 0xffu;
                if (cd == kCellEmpty) continue;
                const int q = tid + r * nt;
                int dv = (int)(cd & 0xfu);
                if (cd == kCellMixed) dv = (int)(pl.vmeta[q] & 0xffu);
                else if ((cd & kCellHoles) && st.plo[r].y == kResHole) dv = 0;
                const uint4 slo = plan_unpack(st.plo[r]), shi = r == 0 ? plan_unpack(st.phi0) : make_uint4(0, 0, 0, 0);
                const unsigned off[8] = {slo.x, slo.y, slo.z, slo.w, shi.x, shi.y, shi.z, shi.w};
                P l = st.l[r];
                if (a.T == 0) {
#pragma unroll
                    for (int g = 0; g < G; ++g) l.x[g] = (T)0;
                }
#pragma unroll
                for (int e = 0; e < (r == 0 ? 8 : 4); ++e)
                    if (e < dv) lds_store<P>(off[e], l);
            }
        }
    } else if constexpr (REG) {
        // the lane's variables q = tid + r*nt: plan entries and LLR pairs into registers, once per launch
        const P *L = reinterpret_cast<const P *>(llr_s);
#pragma unroll
        for (int r = 0; r < kResRegVars; ++r) {
            const int q = tid + r * nt;
            if (q < n) {
                st.meta[r] = pl.vmeta[q];
                st.plo[r] = pl.vslot_lo[q];
                if (r == 0 && q < pl.n_hi) st.phi0 = pl.vslot_hi[q];
                st.l[r] = L[q];
            }
        }
#pragma unroll
        for (int r = 0; r < kResRegVars; ++r) {
            if (tid + r * nt < n) {
                const uint4 slo = plan_unpack(st.plo[r]), shi = r == 0 ? plan_unpack(st.phi0) : make_uint4(0, 0, 0, 0);
                const unsigned off[8] = {slo.x, slo.y, slo.z, slo.w, shi.x, shi.y, shi.z, shi.w};
                const int dv = (int)(st.meta[r] & 0xffu);
                P l = st.l[r];
                if constexpr (!std::is_same<T, float>::value) {
#pragma unroll
                    for (int g = 0; g < G; ++g) l.x[g] = __builtin_canonicalize(l.x[g]);   // quiet NaNs (see the fp64 check phase)
                }
                if (a.T == 0) {
#pragma unroll
                    for (int g = 0; g < G; ++g) l.x[g] = (T)0;
                }
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (e < dv) lds_store<P>(off[e], l);
            }
        }
    } else {
        const P *L = reinterpret_cast<const P *>(llr_s);
        for (int q0 = tid; q0 < n; q0 += kPro * nt) {
            int dvk[kPro];
            uint2 plo[kPro], phi[kPro];
#pragma unroll
            for (int k = 0; k < kPro; ++k) {                       // plan loads of the whole batch first
                const int q = q0 + k * nt;
                dvk[k] = 0;
                plo[k] = make_uint2(0, 0);
                phi[k] = make_uint2(0, 0);
                if (q < n) {
                    dvk[k] = (int)(pl.vmeta[q] & 0xffu);
                    plo[k] = pl.vslot_lo[q];
                    if (q < pl.n_hi) phi[k] = pl.vslot_hi[q];
                }
            }
#pragma unroll
            for (int k = 0; k < kPro; ++k) {
                const int q = q0 + k * nt;
                if (q < n) {
                    const uint4 slo = plan_unpack(plo[k]), shi = plan_unpack(phi[k]);
                    const unsigned off[8] = {slo.x, slo.y, slo.z, slo.w, shi.x, shi.y, shi.z, shi.w};
                    P l = L[q];
                    if constexpr (!std::is_same<T, float>::value) {
#pragma unroll
                        for (int g = 0; g < G; ++g) l.x[g] = __builtin_canonicalize(l.x[g]);   // quiet NaNs (see the fp64 check phase)
                    }
                    if (a.T == 0) {
#pragma unroll
                        for (int g = 0; g < G; ++g) l.x[g] = (T)0;
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (e < dvk[k]) lds_store<P>(off[e], l);
                }
            }
        }
    }
    if constexpr ((EE & kCptEntry) == 0) {
        if constexpr (CPT) chk_cells = pl.ccell[__builtin_amdgcn_readfirstlane(tid) >> 6];
        dc_pre = tid < pl.m ? pl.dc_s[tid] : 0;
        b_pre = (BPC && tid < pl.m && a.T > 0) ? g_beta[pl.bslot_c[tid]] : (T)0;
    }
    __syncthreads();

    unsigned done = 0;                                   // block-uniform
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (b0 + g >= a.batch) done |= 1u << g;

    for (int it = 0; it < a.T; ++it) {
        const T *beta_row = g_beta + (size_t)it * a.n_beta;
        const T *oa_row = a.oms_alpha ? g_oms_alpha + (size_t)it * a.n_oms_alpha : nullptr;
        const float *thr = FORM == FORM_RCQ ? a.thr + (size_t)a.q_of_iter[it] * a.n_levels : nullptr;
        const T *alpha_lds = a.alpha_in_lds ? alpha_s + it * a.n_alpha : nullptr;
        const T *alpha_glb = g_alpha + (size_t)it * a.n_alpha;
        res_check_phase<G, FORM, BPC, NL, MS, T, SPLIT, CPT>(pl, res_smem, beta_row, oa_row, thr, a.n_levels,
                                                             a.rcq_zero0 != 0, dc_pre, b_pre, tid, nt, chk_cells);
        if (BPC && tid < pl.m && it + 1 < a.T) {         // next iteration's beta: in flight across the phases below
            if constexpr (CPT) {
                // the column's address is formed here from the scalar base and an opaque lane offset: hoisted out of the
                // loop it was a 64-bit lane address, spilled and reloaded every iteration
                unsigned p = (unsigned)tid;
                asm volatile("" : "+v"(p));
                b_pre = *res_at(g_beta + (size_t)(it + 1) * a.n_beta, (unsigned)*res_at(pl.bslot_c, p));
            } else {
                b_pre = g_beta[(size_t)(it + 1) * a.n_beta + pl.bslot_c[tid]];
            }
        }
        __syncthreads();
        if (ES && !a.posterior) {
            // reference stop rule without a second gather pass: the variable phase also yields this iteration's
            // hard decisions (the posterior shares the gathered C2V values); outputs are bits only
            const bool last = it == a.T - 1;
            if (last) res_var_phase<G, 1, T, REG>(pl, res_smem, llr_s, bits_s, (const T *)nullptr, (const T *)nullptr, 0u, tid, nt, st, ps);
            else if (a.unit_alpha) res_var_phase<G, 6, T, REG>(pl, res_smem, llr_s, bits_s, (const T *)nullptr, (const T *)nullptr, 0u, tid, nt, st, ps);
            else res_var_phase<G, 4, T, REG>(pl, res_smem, llr_s, bits_s, alpha_lds, alpha_glb, 0u, tid, nt, st, ps);
            __syncthreads();
            // the flag word alternates between iterations: this one's is read after ONE barrier while thread 0 already clears
            // the other one for the next iteration (no third barrier)
            unsigned *su = sh_unsat + (it & 1);
            if (ps.par_off) res_parity_reduce<G, SPLIT>(pl, ps.par_off, su, tid, nt);    // the variable lanes scattered the parities
            else res_syndrome_phase<G, SPLIT>(pl, bits_s, su, tid, nt);
            __syncthreads();
            const unsigned unsat = *su;
            if (tid == 0) sh_unsat[(it + 1) & 1] = 0;
            const unsigned newly = ~unsat & ~done & kAll;
            if (newly) {                                 // block-uniform
                res_emit_bits<G>(pl, a, bits_s, b0, newly, it + 1, 0u, tid, nt);
                done |= newly;
                if (done == kAll) return;
                __syncthreads();                         // bits_s is rewritten by the next iteration
            }
            continue;
        }
        if (ES) {
            res_var_phase<G, 1, T, REG>(pl, res_smem, llr_s, bits_s, (const T *)nullptr, (const T *)nullptr, 0u, tid, nt, st, ps);
            __syncthreads();
            unsigned *su = sh_unsat + (it & 1);
            if (ps.par_off) res_parity_reduce<G, SPLIT>(pl, ps.par_off, su, tid, nt);
            else res_syndrome_phase<G, SPLIT>(pl, bits_s, su, tid, nt);
            __syncthreads();
            const unsigned unsat = *su;
            if (tid == 0) sh_unsat[(it + 1) & 1] = 0;
            const unsigned newly = ~unsat & ~done & kAll;
            if (newly) {                                 // block-uniform
                if (a.dbg_c2v) res_dump_c2v<G, T>(pl, a, b0, newly, tid, nt);      // slots still hold this iteration's C2V
                res_var_phase<G, 1, T, REG>(pl, res_smem, llr_s, bits_s, (const T *)nullptr, (const T *)nullptr, newly, tid, nt, st);
                __syncthreads();
                res_emit<G, T>(pl, a, llr_s, b0, newly, it + 1, 0u, tid, nt);
                done |= newly;
                if (done == kAll) return;                // every codeword of the block has its outputs
                __syncthreads();
            }
        }
        if (it != a.T - 1) {
            if (a.unit_alpha) res_var_phase<G, 2, T, REG, CPT>(pl, res_smem, llr_s, bits_s, (const T *)nullptr, (const T *)nullptr, 0u, tid, nt, st);
            else res_var_phase<G, 0, T, REG, CPT>(pl, res_smem, llr_s, bits_s, alpha_lds, alpha_glb, 0u, tid, nt, st);
            __syncthreads();
        }
    }

    // codewords still open after T iterations: outputs of the last iteration
    const unsigned open = ~done & kAll;
    if (!open) return;
    if (a.dbg_c2v) {                                     // slots hold the C2V of iteration T-1 (zeros when T == 0)
        unsigned real = 0;
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (b0 + g < a.batch) real |= 1u << g;
        res_dump_c2v<G, T>(pl, a, b0, open & real, tid, nt);
        __syncthreads();                                 // the final posterior pass overwrites the slots
    }
    if (ES && !a.posterior && a.T > 0) {                 // bits_s hold iteration T's decisions already
        res_emit_bits<G>(pl, a, bits_s, b0, open, a.T, kAll, tid, nt);
        return;
    }
    // fixed-T mode: success = final syndrome is zero.  With parity words (power-of-two stride) the posterior pass scatters the
    // decisions into them (one LDS atomic per edge, then m words are read); otherwise the decisions go into the dead message
    // slots and every check reads its row of them back (MODE 8 / res_syndrome_slots)
    const bool scatter = !ES && !CPT && psf.par_off != 0;   // compact plans: odd row stride, no parity words
    if (ES) res_var_phase<G, 1, T, REG>(pl, res_smem, llr_s, bits_s, (const T *)nullptr, (const T *)nullptr, open, tid, nt, st);
    else if (scatter) res_var_phase<G, 1, T, REG>(pl, res_smem, llr_s, bits_s, (const T *)nullptr, (const T *)nullptr, open, tid, nt, st, psf);
    else res_var_phase<G, CPT ? 9 : 8, T, REG, CPT>(pl, res_smem, llr_s, bits_s, (const T *)nullptr, (const T *)nullptr, open, tid, nt, st);
    if constexpr ((EE & kCptExit) != 0) {
        // a full block's inverse-permutation entries are issued here, ahead of the three barriers below instead of behind them.
        // The block's form and the wave's base are worked out again (scalar unit) instead of living across the iterations
        unsigned ip[kCptRows] = {};
        cpt_fast = res_cpt_full_block<G>(pl, a, b0);
        const unsigned wbase = (unsigned)__builtin_amdgcn_readfirstlane(tid) & ~63u;
        if (cpt_fast) {
#pragma unroll
            for (int k = 0; k < kCptRows; ++k)
                ip[k] = *res_at(pl.inv_perm_v, min((unsigned)tid + (unsigned)(k * kResCptThreads), (unsigned)n - 1u));
        }
        __syncthreads();
        res_cpt_syndrome_slots<G, MS>(chk_cells, dc_pre, sh_unsat, tid);
        __syncthreads();
        const unsigned unsat = *sh_unsat;
        // the slots are dead now: the posteriors the last pass kept in registers go to the staging rows (sorted order);
        // a cell without holes stores unmasked
#pragma unroll
        for (int r = 0; r < kResRegVars; ++r) {
            const unsigned cd = (st.cells >> (8 * r)) & 0xffu;
            const unsigned q = (unsigned)tid + (unsigned)(r * kResCptThreads);
            if (cd == kCellEmpty) continue;
            if (cd != kCellMixed && !(cd & kCellHoles)) lds_store<P>(q * (unsigned)sizeof(P), st.l[r]);
            else if (q < (unsigned)pl.n_pos) lds_store<P>(q * (unsigned)sizeof(P), st.l[r]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kCptRows; ++k) asm volatile("" : "+v"(ip[k]));   // nothing waits for the entries before this point
        if (cpt_fast) res_cpt_emit<G>(pl, a, b0, ip, a.T, unsat, tid, wbase);
        else res_emit<G, T>(pl, a, llr_s, b0, open, a.T, unsat, tid, nt);
        return;
    }
    __syncthreads();
    unsigned unsat = kAll;
    if (!ES) {
        if (scatter) res_parity_reduce<G, SPLIT>(pl, psf.par_off, sh_unsat, tid, nt);
        else res_syndrome_slots<G, T, SPLIT>(pl, sh_unsat, tid, nt);
        __syncthreads();
        unsat = *sh_unsat;
    }
    if constexpr (CPT) {
        // the slots are dead now: the posteriors the last pass kept in registers go to the staging rows (sorted order)
#pragma unroll
        for (int r = 0; r < kResRegVars; ++r)
            if (tid + r * nt < pl.n_pos) reinterpret_cast<P *>(llr_s)[tid + r * nt] = st.l[r];
        __syncthreads();
    }
    res_emit<G, T>(pl, a, llr_s, b0, open, a.T, unsat, tid, nt);
}

}  // namespace ldpc
