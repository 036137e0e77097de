// ldpc_constellation.hip -- the symbol channel on a constellation given as a table: up to 64 labelled points in the plane
// (8-PSK, APSK, any labelling, rotated, shaped or learned sets) over AWGN or per-symbol Rayleigh fading, demapped jointly over
// all points with the max-log or the exact rule (ldpc_channel_con), the training draw (ldpc_channel_con_mix), LLRs from
// received samples (ldpc_demap_con), extrinsic LLRs from samples and a priori LLRs (ldpc_demap_con_prior) and one SNR point
// (ldpc_simulate_con) of include/ldpc_hip.h.
//
// Included by ldpc_hip.hip below ldpc_modulation.hip: it uses that file's lane arithmetic (sym_lane), codeword bit extraction
// (sym_bits), stores (sym_put / sym_store), counter tag, demapper check and simulate loop.  Still the one compiled unit.
//
// Definition (include/ldpc_hip.h; tests/constellation_reference.py restates it in numpy).  The frame layout,
// the interleaver, the pad bits and the Philox counters are the symbol channel's.  The symbol's label is l = sum_k b_k 2^k, the
// `bits` word sym_bits forms; the sent point is points[l] = (xI, xQ).
//   e = g * amp;  vI = e * xI_l + zI;  vQ = e * xQ_l + zQ
//   for c = 0 .. 2^m - 1:  tI = vI - e * xI_c;  tQ = vQ - e * xQ_c;  D_c = tI * tI + tQ * tQ
//   m_b(k) = min over c with bit k of c equal to b of D_c;   max-log:  llr_k = 0.5f * (m_1 - m_0)
//   exact:  S_b = sum_{c: bit k = b, ascending c} expf(-0.5f * (D_c - m_b));  llr_k = 0.5f * (m_1 - m_0) + (logf(S_0) - logf(S_1))
// Every multiply and add is rounded on its own: no fmaf is written here and the unit is built with -ffp-contract=off.
//
// The table (at most 64 points, 512 bytes) is wave-uniform.  Each workgroup stages it once in LDS; the candidate loop is fully
// unrolled and reads it at compile-time offsets (every lane the same address: a broadcast), the sent point at the lane's label.
// The exact rule keeps the 2^m distances in registers (compile-time indices after unrolling); see
// profiles/constellation_compiler_report.txt for what that costs.

namespace ldpc {

constexpr int kConMaxBits = 6;

// the workgroup's copy of the table; every lane of the workgroup takes part, lanes past the block included
template <int M>
__device__ inline void con_stage(float2 *tab, const float2 *__restrict__ points)
{
    static_assert((1 << M) <= kSimBlock, "one lane per point");
    if (threadIdx.x < (1u << M)) tab[threadIdx.x] = points[threadIdx.x];
    __syncthreads();
}

// LLRs of one received sample (vI, vQ) at gain e: the one rule behind the channel kernels and con_demap, so a sample that a
// channel kernel stored demaps to the LLRs that kernel stored, bit for bit
template <int M, bool EXACT>
__device__ inline void con_rule(float vI, float vQ, float e, const float2 *tab, float (&llr)[M])
{
    constexpr int L = 1 << M;
    float m0[M], m1[M];
#pragma unroll
    for (int k = 0; k < M; ++k) m0[k] = m1[k] = INFINITY;
    float D[EXACT ? L : 1];
    (void)D;
#pragma unroll
    for (int c = 0; c < L; ++c) {
        const float2 x = tab[c];
        const float eI = e * x.x;
        const float eQ = e * x.y;
        const float tI = vI - eI;
        const float tQ = vQ - eQ;
        const float qI = tI * tI;
        const float qQ = tQ * tQ;
        const float d = qI + qQ;
        if constexpr (EXACT) D[c] = d;
#pragma unroll
        for (int k = 0; k < M; ++k) {
            if ((c >> k) & 1) m1[k] = fminf(m1[k], d);
            else m0[k] = fminf(m0[k], d);
        }
    }
#pragma unroll
    for (int k = 0; k < M; ++k) {
        const float diff = m1[k] - m0[k];
        if constexpr (EXACT) {
            float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
            for (int c = 0; c < L; ++c) {
                if ((c >> k) & 1) {
                    const float x = D[c] - m1[k];
                    s1 = s1 + expf(-0.5f * x);
                } else {
                    const float x = D[c] - m0[k];
                    s0 = s0 + expf(-0.5f * x);
                }
            }
            const float corr = logf(s0) - logf(s1);
            llr[k] = 0.5f * diff + corr;
        } else {
            llr[k] = 0.5f * diff;
        }
    }
}

// the symbol's draw: the counters, normals and fading gain of sim_channel_sym, the labelled point through v = e * x + z
template <bool FADING>
__device__ inline void con_send(const float2 *tab, unsigned bits, unsigned long long f, unsigned s, uint32_t stream_id,
                                uint32_t k0, uint32_t k1, float amp, float &vI, float &vQ, float &e)
{
    uint32_t x[4];
    philox4x32_10((uint32_t)f, (uint32_t)(f >> 32), kSymCounterTag | s, stream_id, k0, k1, x);
    float zI, zQ;
    sim_box_muller(x[0], x[1], zI, zQ);
    float g = 1.0f;
    if (FADING) g = sqrtf(-logf(sim_uniform(x[2])));
    e = g * amp;
    const float2 pt = tab[bits];
    const float eI = e * pt.x;
    const float eQ = e * pt.y;
    vI = eI + zI;
    vQ = eQ + zQ;
}

// LLRs from received samples (ldpc_demap_con): sym_demap with the joint rule
template <int M, bool PERM, bool EXACT>
__global__ __launch_bounds__(kSimBlock) void con_demap(float *__restrict__ llr, long long batch, int n, unsigned S,
                                                       const int *__restrict__ pos, const float4 *__restrict__ received,
                                                       const float2 *__restrict__ points)
{
    __shared__ float2 tab[1 << M];
    con_stage<M>(tab, points);
    long long b;
    unsigned s;
    sym_lane(S, b, s);
    if (b >= batch) return;
    const int j0 = (int)s * M;                                                    // < n <= 2^31 - 1
    const int cnt = n - j0 < M ? n - j0 : M;
    const float4 r = received[(size_t)b * S + s];
    float v[M];
    con_rule<M, EXACT>(r.x, r.y, r.z, tab, v);
    int p[M];
    (void)p;
    if constexpr (PERM) {
#pragma unroll
        for (int k = 0; k < M; ++k) p[k] = k < cnt ? pos[j0 + k] : 0;
    }
    sym_put<M, PERM>(llr + (size_t)b * (size_t)n, p, j0, cnt, v);
}

// extrinsic LLRs of one received sample given the a priori LLRs la[k] of its bits (ldpc_demap_con_prior).  A_c is the sum of
// la over the set bits of c: one add per candidate onto the sum of c without its highest set bit, all indices compile-time
// after unrolling.  Lam_c = D_c + 2.0f * A_c is D_c exactly when every la is +-0.0f, so the rule is then con_rule's bit for
// bit.  con_rule itself is left alone: the kernels built on it compile to what they compiled to before.
template <int M, bool EXACT>
__device__ inline void con_rule_prior(float vI, float vQ, float e, const float2 *tab, const float (&la)[M], float (&llr)[M])
{
    constexpr int L = 1 << M;
    float m0[M], m1[M];
#pragma unroll
    for (int k = 0; k < M; ++k) m0[k] = m1[k] = INFINITY;
    float A[L];                                            // max-log: dead once Lam_c is formed;  exact: Lam_c takes its place
    A[0] = 0.0f;
#pragma unroll
    for (int c = 1; c < L; ++c) {
        const int h = 31 - __builtin_clz((unsigned)c);     // the highest set bit of c
        A[c] = A[c - (1 << h)] + la[h];
    }
#pragma unroll
    for (int c = 0; c < L; ++c) {
        const float2 x = tab[c];
        const float eI = e * x.x;
        const float eQ = e * x.y;
        const float tI = vI - eI;
        const float tQ = vQ - eQ;
        const float qI = tI * tI;
        const float qQ = tQ * tQ;
        const float d = qI + qQ;
        const float a2 = 2.0f * A[c];
        const float lam = d + a2;
        if constexpr (EXACT) A[c] = lam;
#pragma unroll
        for (int k = 0; k < M; ++k) {
            if ((c >> k) & 1) m1[k] = fminf(m1[k], lam);
            else m0[k] = fminf(m0[k], lam);
        }
    }
#pragma unroll
    for (int k = 0; k < M; ++k) {
        const float diff = m1[k] - m0[k];
        if constexpr (EXACT) {
            float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
            for (int c = 0; c < L; ++c) {
                if ((c >> k) & 1) {
                    const float x = A[c] - m1[k];
                    s1 = s1 + expf(-0.5f * x);
                } else {
                    const float x = A[c] - m0[k];
                    s0 = s0 + expf(-0.5f * x);
                }
            }
            const float corr = logf(s0) - logf(s1);
            const float post = 0.5f * diff + corr;
            llr[k] = post - la[k];
        } else {
            llr[k] = 0.5f * diff - la[k];
        }
    }
}

// extrinsic LLRs from received samples and a priori LLRs (ldpc_demap_con_prior): con_demap with con_rule_prior.  A lane loads
// the priors of its own symbol's variables only, all of them before its first store, and stores to those variables only: llr
// may be prior or prior_sub themselves (none of the three is __restrict__).  Pad bits have the prior +0.0f.
template <int M, bool PERM, bool EXACT>
__global__ __launch_bounds__(kSimBlock) void con_demap_prior(float *llr, long long batch, int n, unsigned S,
                                                             const int *__restrict__ pos, const float4 *__restrict__ received,
                                                             const float2 *__restrict__ points, const float *prior,
                                                             const float *prior_sub, float prior_scale)
{
    __shared__ float2 tab[1 << M];
    con_stage<M>(tab, points);
    long long b;
    unsigned s;
    sym_lane(S, b, s);
    if (b >= batch) return;
    const int j0 = (int)s * M;                                                    // < n <= 2^31 - 1
    const int cnt = n - j0 < M ? n - j0 : M;
    const float4 r = received[(size_t)b * S + s];
    int p[M];
    (void)p;
    if constexpr (PERM) {
#pragma unroll
        for (int k = 0; k < M; ++k) p[k] = k < cnt ? pos[j0 + k] : 0;
    }
    const size_t row = (size_t)b * (size_t)n;
    float la[M];
#pragma unroll
    for (int k = 0; k < M; ++k) {
        la[k] = 0.0f;
        if (k < cnt) {
            const size_t j = row + (size_t)(PERM ? p[k] : j0 + k);
            const float a = prior_sub ? prior[j] - prior_sub[j] : prior[j];
            la[k] = prior_scale * a;
        }
    }
    float v[M];
    con_rule_prior<M, EXACT>(r.x, r.y, r.z, tab, la, v);
    sym_put<M, PERM>(llr + row, p, j0, cnt, v);
}

// sim_channel_sym on a table: the same lanes, bits, counters and stores, con_send and con_rule where sym_axis stands
template <int M, bool FADING, bool PERM, bool EXACT>
__global__ __launch_bounds__(kSimBlock) void sim_channel_con(float *__restrict__ llr, long long batch, int n, unsigned S,
                                                             uint32_t k0, uint32_t k1, uint32_t stream_id,
                                                             unsigned long long first_frame, float amp,
                                                             const int *__restrict__ pos, const uint8_t *__restrict__ cw,
                                                             long long cw_stride, float4 *__restrict__ received,
                                                             const float2 *__restrict__ points)
{
    __shared__ float2 tab[1 << M];
    con_stage<M>(tab, points);
    long long b;
    unsigned s;
    sym_lane(S, b, s);
    if (b >= batch) return;
    const int j0 = (int)s * M;                                                    // < n <= 2^31 - 1
    const int cnt = n - j0 < M ? n - j0 : M;
    const int rb = (n + 7) >> 3;
    const uint8_t *row = cw ? cw + (size_t)b * (size_t)cw_stride : nullptr;
    int p[M];                                                                     // permuted path: the symbol's variables
    (void)p;
    const unsigned bits = sym_bits<M, PERM>(row, pos, j0, cnt, rb, p);            // the label; pad bits 0
    float vI, vQ, e;
    con_send<FADING>(tab, bits, first_frame + (unsigned long long)b, s, stream_id, k0, k1, amp, vI, vQ, e);
    float v[M];
    con_rule<M, EXACT>(vI, vQ, e, tab, v);
    if (received) received[(size_t)b * S + s] = make_float4(vI, vQ, e, 0.0f);
    sym_put<M, PERM>(llr + (size_t)b * (size_t)n, p, j0, cnt, v);
}

// sim_channel_sym_mix on a table: amp = amp_tab[(first_frame + b) mod K] by that kernel's remainder, the sent bits as targets
template <int M, bool FADING, bool PERM, bool EXACT>
__global__ __launch_bounds__(kSimBlock) void sim_channel_con_mix(float *__restrict__ llr, float *__restrict__ targets,
                                                                 long long batch, int n, unsigned S, uint32_t k0, uint32_t k1,
                                                                 uint32_t stream_id, unsigned long long first_frame,
                                                                 unsigned p0, unsigned K, unsigned Kinv,
                                                                 const float *__restrict__ amp_tab,
                                                                 const int *__restrict__ pos, const uint8_t *__restrict__ cw,
                                                                 long long cw_stride, const float2 *__restrict__ points)
{
    __shared__ float2 tab[1 << M];
    con_stage<M>(tab, points);
    long long b;
    unsigned s;
    sym_lane(S, b, s);
    if (b >= batch) return;
    const unsigned r = (unsigned)b + p0;
    unsigned pt = r - __umulhi(r, Kinv) * K;                                      // in [0, 2K), as in sim_channel_awgn_mix
    if (pt >= K) pt -= K;                                                         // (first_frame + b) mod K
    const float amp = amp_tab[pt];
    const int j0 = (int)s * M;                                                    // < n <= 2^31 - 1
    const int cnt = n - j0 < M ? n - j0 : M;
    const int rb = (n + 7) >> 3;
    const uint8_t *row = cw ? cw + (size_t)b * (size_t)cw_stride : nullptr;
    int p[M];                                                                     // permuted path: the symbol's variables
    (void)p;
    const unsigned bits = sym_bits<M, PERM>(row, pos, j0, cnt, rb, p);            // the label; pad bits 0
    float vI, vQ, e;
    con_send<FADING>(tab, bits, first_frame + (unsigned long long)b, s, stream_id, k0, k1, amp, vI, vQ, e);
    float v[M];
    con_rule<M, EXACT>(vI, vQ, e, tab, v);
    sym_put<M, PERM>(llr + (size_t)b * (size_t)n, p, j0, cnt, v);
    if (targets) {
        float sent[M];
#pragma unroll
        for (int k = 0; k < M; ++k) sent[k] = ((bits >> k) & 1u) ? 1.0f : 0.0f;
        sym_put<M, PERM>(targets + (size_t)b * (size_t)n, p, j0, cnt, sent);
    }
}

}  // namespace ldpc

namespace {

// the scalar part of a constellation descriptor, in the order include/ldpc_hip.h states; the position table and the
// contents of `points` are device memory the caller vouches for.  The S < 2^29 check comes after the entry's other scalars
// (con_symbols_check).
int con_desc_check(const ldpc_constellation *con, bool check_fading = true, bool check_amp = true)
{
    if (!con) return fail(LDPC_ERR_ARG, "NULL con");
    const int32_t m = con->bits_per_symbol;
    if (m < 1 || m > kConMaxBits) return fail(LDPC_ERR_ARG, "bits_per_symbol must be in 1 .. 6 (2 .. 64 points), got %d", m);
    if (!con->points) return fail(LDPC_ERR_ARG, "NULL points");
    if (check_fading && con->fading != 0 && con->fading != 1)
        return fail(LDPC_ERR_ARG, "fading must be 0 (none) or 1 (Rayleigh per symbol), got %d", con->fading);
    if (check_amp && !(std::isfinite(con->amp) && con->amp >= 0.0f)) return fail(LDPC_ERR_ARG, "amp must be finite and >= 0");
    return LDPC_OK;
}

int con_stride_check(int64_t codeword_stride, int32_t n)
{
    if (codeword_stride != 0 && codeword_stride != ((int64_t)n + 7) / 8)
        return fail(LDPC_ERR_ARG, "codeword_stride must be 0 (one codeword) or ceil(n / 8) = %lld (one packed row per frame)",
                    (long long)(((int64_t)n + 7) / 8));
    return LDPC_OK;
}

int con_symbols_check(const ldpc_constellation *con, int32_t n)
{
    const int64_t S = ((int64_t)n + con->bits_per_symbol - 1) / con->bits_per_symbol;
    if (S >= (int64_t)kSymMaxSymbols)
        return fail(LDPC_ERR_UNSUPPORTED, "a frame of %lld symbols: the symbol index must stay below 2^29", (long long)S);
    return LDPC_OK;
}

int con_points_check(const ldpc_constellation *con)
{
    if (((uintptr_t)con->points % 8) != 0) return fail(LDPC_ERR_ARG, "points must be 8-byte aligned");
    return LDPC_OK;
}

// one bit per symbol has one point per set: both sums are 1.0f and the exact rule is the max-log rule bit for bit
inline bool con_exact(int32_t demapper, int m) { return demapper == LDPC_DEMAP_EXACT && m >= 2; }

int con_grid(int64_t batch, unsigned S, dim3 &grid)
{
    const unsigned long long syms = (unsigned long long)batch * S;
    const unsigned long long blocks = (syms + kSimBlock - 1) / kSimBlock;
    if (blocks > 0x7fffffffull) return fail(LDPC_ERR_UNSUPPORTED, "batch too large for one launch");
    grid = dim3((unsigned)blocks);
    return LDPC_OK;
}

struct ConArgs {
    float *llr, *targets;
    long long batch;
    int n;
    unsigned S;
    uint32_t k0, k1, stream_id;
    unsigned long long first_frame;
    float amp;
    unsigned p0, K, Kinv;
    const float *amp_tab;
    const int *pos;
    const uint8_t *cw;
    long long cw_stride;
    float4 *received;
    const float2 *points;
    const float *prior, *prior_sub;
    float prior_scale;
};

enum { kConChannel, kConMix, kConDemap, kConDemapPrior };

template <int KIND, int M, bool FADING, bool PERM, bool EXACT>
void con_launch_one(dim3 grid, hipStream_t s, const ConArgs &a)
{
    if constexpr (KIND == kConChannel)
        hipLaunchKernelGGL((sim_channel_con<M, FADING, PERM, EXACT>), grid, dim3(kSimBlock), 0, s, a.llr, a.batch, a.n, a.S, a.k0, a.k1,
                           a.stream_id, a.first_frame, a.amp, a.pos, a.cw, a.cw_stride, a.received, a.points);
    else if constexpr (KIND == kConMix)
        hipLaunchKernelGGL((sim_channel_con_mix<M, FADING, PERM, EXACT>), grid, dim3(kSimBlock), 0, s, a.llr, a.targets, a.batch, a.n,
                           a.S, a.k0, a.k1, a.stream_id, a.first_frame, a.p0, a.K, a.Kinv, a.amp_tab, a.pos, a.cw, a.cw_stride,
                           a.points);
    else if constexpr (KIND == kConDemap)
        hipLaunchKernelGGL((con_demap<M, PERM, EXACT>), grid, dim3(kSimBlock), 0, s, a.llr, a.batch, a.n, a.S, a.pos,
                           (const float4 *)a.received, a.points);
    else
        hipLaunchKernelGGL((con_demap_prior<M, PERM, EXACT>), grid, dim3(kSimBlock), 0, s, a.llr, a.batch, a.n, a.S, a.pos,
                           (const float4 *)a.received, a.points, a.prior, a.prior_sub, a.prior_scale);
}

template <int KIND, int M, bool EXACT>
void con_launch_m(bool fading, bool perm, dim3 grid, hipStream_t s, const ConArgs &a)
{
    constexpr bool kDraws = KIND != kConDemap && KIND != kConDemapPrior;
    if (kDraws && fading) {                                // the demappers read the gain out of the samples: one form for both
        if (perm) con_launch_one<KIND, M, kDraws, true, EXACT>(grid, s, a);
        else con_launch_one<KIND, M, kDraws, false, EXACT>(grid, s, a);
    } else {
        if (perm) con_launch_one<KIND, M, false, true, EXACT>(grid, s, a);
        else con_launch_one<KIND, M, false, false, EXACT>(grid, s, a);
    }
}

// one launch of a constellation kernel; con has passed its checks, 1 <= m <= 6
template <int KIND>
int con_launch(const ldpc_constellation *con, int32_t demapper, hipStream_t s, ConArgs a)
{
    const int m = con->bits_per_symbol;
    a.S = (unsigned)(((int64_t)a.n + m - 1) / m);
    a.pos = (const int *)con->position;
    a.points = (const float2 *)con->points;
    dim3 grid;
    if (int rc = con_grid(a.batch, a.S, grid)) return rc;
    const bool perm = con->position != nullptr, fading = con->fading != 0;
    if (con_exact(demapper, m)) {
        switch (m) {
        case 2: con_launch_m<KIND, 2, true>(fading, perm, grid, s, a); break;
        case 3: con_launch_m<KIND, 3, true>(fading, perm, grid, s, a); break;
        case 4: con_launch_m<KIND, 4, true>(fading, perm, grid, s, a); break;
        case 5: con_launch_m<KIND, 5, true>(fading, perm, grid, s, a); break;
        case 6: con_launch_m<KIND, 6, true>(fading, perm, grid, s, a); break;
        default: return fail(LDPC_ERR_ARG, "bits_per_symbol %d", m);
        }
    } else {
        switch (m) {
        case 1: con_launch_m<KIND, 1, false>(fading, perm, grid, s, a); break;
        case 2: con_launch_m<KIND, 2, false>(fading, perm, grid, s, a); break;
        case 3: con_launch_m<KIND, 3, false>(fading, perm, grid, s, a); break;
        case 4: con_launch_m<KIND, 4, false>(fading, perm, grid, s, a); break;
        case 5: con_launch_m<KIND, 5, false>(fading, perm, grid, s, a); break;
        case 6: con_launch_m<KIND, 6, false>(fading, perm, grid, s, a); break;
        default: return fail(LDPC_ERR_ARG, "bits_per_symbol %d", m);
        }
    }
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int sim_channel_con_launch(float *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                           const ldpc_constellation *con, int32_t demapper, const uint8_t *cw, int64_t cw_stride, void *received,
                           hipStream_t s)
{
    ConArgs a{};
    a.llr = llr, a.batch = (long long)batch, a.n = (int)n;
    a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32), a.stream_id = stream_id, a.first_frame = (unsigned long long)first_frame;
    a.amp = con->amp, a.cw = cw, a.cw_stride = (long long)cw_stride, a.received = (float4 *)received;
    return con_launch<kConChannel>(con, demapper, s, a);
}

}  // namespace

extern "C" {

int ldpc_channel_con(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                     const ldpc_constellation *con, const uint8_t *codewords_packed, int64_t codeword_stride, void *received,
                     int32_t demapper, void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (int rc = con_desc_check(con)) return rc;
    if (int rc = con_stride_check(codeword_stride, n)) return rc;
    if (int rc = sym_demapper_check(demapper)) return rc;
    if (int rc = con_symbols_check(con, n)) return rc;
    if (batch == 0) return LDPC_OK;
    if (!llr) return fail(LDPC_ERR_ARG, "NULL llr");
    if (((uintptr_t)llr % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "llr must be 4-byte aligned");
    if (received && ((uintptr_t)received % 16) != 0) return fail(LDPC_ERR_ARG, "received must be 16-byte aligned");
    if (int rc = con_points_check(con)) return rc;
    return sim_channel_con_launch((float *)llr, batch, n, seed, stream_id, first_frame, con, demapper, codewords_packed,
                                  codeword_stride, received, (hipStream_t)stream);
}

int ldpc_channel_con_mix(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                         const ldpc_constellation *con, const float *amp_tab, int32_t n_points, const uint8_t *codewords_packed,
                         int64_t codeword_stride, void *targets, int32_t demapper, void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (int rc = con_desc_check(con, true, false)) return rc;
    if (int rc = con_stride_check(codeword_stride, n)) return rc;
    if (int rc = sym_demapper_check(demapper)) return rc;
    if (n_points < 1 || n_points > 4096) return fail(LDPC_ERR_ARG, "n_points must be in 1 .. 4096");
    if (batch > INT32_MAX) return fail(LDPC_ERR_ARG, "batch > 2^31 - 1");
    if (batch > 0 && first_frame > (uint64_t)0 - (uint64_t)batch)       // 2^64 - batch: the point index is not continuous across the wrap
        return fail(LDPC_ERR_ARG, "first_frame + batch wraps the 64-bit frame index");
    if (batch > 0 && !amp_tab) return fail(LDPC_ERR_ARG, "NULL amp_tab");
    if (int rc = con_symbols_check(con, n)) return rc;
    if (batch == 0) return LDPC_OK;
    if (!llr) return fail(LDPC_ERR_ARG, "NULL llr");
    if (((uintptr_t)llr % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "llr must be 4-byte aligned");
    if (targets && ((uintptr_t)targets % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "targets must be 4-byte aligned");
    if (((uintptr_t)amp_tab % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "amp_tab must be 4-byte aligned");
    if (int rc = con_points_check(con)) return rc;
    const unsigned K = (unsigned)n_points;
    ConArgs a{};
    a.llr = (float *)llr, a.targets = (float *)targets, a.batch = (long long)batch, a.n = (int)n;
    a.k0 = (uint32_t)seed, a.k1 = (uint32_t)(seed >> 32), a.stream_id = stream_id, a.first_frame = (unsigned long long)first_frame;
    a.p0 = (unsigned)(first_frame % K), a.K = K, a.Kinv = 0xffffffffu / K, a.amp_tab = amp_tab;
    a.cw = codewords_packed, a.cw_stride = (long long)codeword_stride;
    return con_launch<kConMix>(con, demapper, (hipStream_t)stream, a);
}

int ldpc_demap_con(void *llr, int64_t batch, int32_t n, const ldpc_constellation *con, int32_t demapper, const void *received,
                   void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (int rc = con_desc_check(con, false, false)) return rc;
    if (int rc = sym_demapper_check(demapper)) return rc;
    if (int rc = con_symbols_check(con, n)) return rc;
    if (batch == 0) return LDPC_OK;
    if (!llr) return fail(LDPC_ERR_ARG, "NULL llr");
    if (((uintptr_t)llr % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "llr must be 4-byte aligned");
    if (!received) return fail(LDPC_ERR_ARG, "NULL received");
    if (((uintptr_t)received % 16) != 0) return fail(LDPC_ERR_ARG, "received must be 16-byte aligned");
    if (int rc = con_points_check(con)) return rc;
    ConArgs a{};
    a.llr = (float *)llr, a.batch = (long long)batch, a.n = (int)n;
    a.received = (float4 *)const_cast<void *>(received);
    return con_launch<kConDemap>(con, demapper, (hipStream_t)stream, a);
}

int ldpc_demap_con_prior(void *llr, int64_t batch, int32_t n, const ldpc_constellation *con, int32_t demapper,
                         const void *received, const void *prior, const void *prior_sub, float prior_scale, void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (int rc = con_desc_check(con, false, false)) return rc;
    if (int rc = sym_demapper_check(demapper)) return rc;
    if (!std::isfinite(prior_scale)) return fail(LDPC_ERR_ARG, "prior_scale must be finite");
    if (int rc = con_symbols_check(con, n)) return rc;
    if (batch == 0) return LDPC_OK;
    if (!llr) return fail(LDPC_ERR_ARG, "NULL llr");
    if (((uintptr_t)llr % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "llr must be 4-byte aligned");
    if (!received) return fail(LDPC_ERR_ARG, "NULL received");
    if (((uintptr_t)received % 16) != 0) return fail(LDPC_ERR_ARG, "received must be 16-byte aligned");
    if (prior && ((uintptr_t)prior % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "prior must be 4-byte aligned");
    if (prior_sub && ((uintptr_t)prior_sub % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "prior_sub must be 4-byte aligned");
    if (prior_sub && !prior) return fail(LDPC_ERR_ARG, "prior_sub without a prior");
    if (int rc = con_points_check(con)) return rc;
    ConArgs a{};
    a.llr = (float *)llr, a.batch = (long long)batch, a.n = (int)n;
    a.received = (float4 *)const_cast<void *>(received);
    if (!prior) return con_launch<kConDemap>(con, demapper, (hipStream_t)stream, a);     // no priors: ldpc_demap_con's kernel
    a.prior = (const float *)prior, a.prior_sub = (const float *)prior_sub, a.prior_scale = prior_scale;
    return con_launch<kConDemapPrior>(con, demapper, (hipStream_t)stream, a);
}

int ldpc_simulate_con(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_encoder *e, const ldpc_constellation *con,
                      int32_t demapper, int64_t capture, int64_t out_state[8], int64_t *out_diag, void *workspace,
                      size_t workspace_bytes, void *stream)
{
    LDPC_NOTHROW(simulate_symbols_impl(
        d, desc, e, "ldpc_simulate_con",
        [&](int32_t n) {
            if (int rc = con_desc_check(con)) return rc;
            if (int rc = sym_demapper_check(demapper)) return rc;
            if (int rc = con_symbols_check(con, n)) return rc;
            return con_points_check(con);
        },
        [&](float *llr, int64_t frames, uint64_t first, const uint8_t *cw, int64_t stride, hipStream_t s) {
            return sim_channel_con_launch(llr, frames, d->g->n, desc->seed, desc->stream_id, first, con, demapper, cw, stride,
                                          nullptr, s);
        },
        capture < 0 ? -1 : capture, out_state, out_diag, workspace, workspace_bytes, stream))
}

}  // extern "C"
