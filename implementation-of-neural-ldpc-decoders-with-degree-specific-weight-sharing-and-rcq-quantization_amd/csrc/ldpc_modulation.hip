// ldpc_modulation.hip -- a symbol channel for the on-device Monte-Carlo path: Gray-mapped BPSK / QPSK / 16- / 64- / 256-QAM over
// AWGN or per-symbol Rayleigh fading with a max-log demapper (ldpc_channel_sym), the host loop of one SNR point on it
// (ldpc_simulate_sym) and the training draw with one SNR point per frame and the sent bits as targets (ldpc_channel_sym_mix)
// of include/ldpc_hip.h.
//
// Included by ldpc_hip.hip below ldpc_encode.hip (it uses ldpc_sim.hip's Philox rounds, uniforms, Box-Muller, counters and
// workspace carving and ldpc_encode.hip's encoder launch and row XOR): still the one compiled unit.
//
// Definition (include/ldpc_hip.h; tests/modulation_reference.py restates it in numpy).  m bits per symbol,
// S = ceil(n / m) symbols per frame, transmit index t = s * m + k is bit k of symbol s and carries the codeword bit of variable
// pos[t] (identity when pos is NULL); transmit indices >= n are pad bits, sent as 0 and never stored.  The first h = m / 2 bits
// label the I axis, the next h the Q axis (m = 1: an I axis with h = 1 only).  An axis is Gray-labelled 2^h-PAM: level index
// i = running XOR of b_0 .. b_{h-1} (b_0 the most significant bit), integer amplitude a = (2^h - 1) - 2 i.
//   (x0, x1, x2, x3) = Philox4x32-10(counter = (f lo, f hi, 0x40000000 | s, stream_id), key = seed)
//   (zI, zQ) = sim_box_muller(x0, x1);  g = 1.0f, or sqrtf(-logf(u(x2))) under Rayleigh fading;  e = g * amp
//   per axis: v = e * (float)a + z;  D(a') = (v - e * (float)a')^2;  llr_k = 0.5f * (min_{b_k = 1} D - min_{b_k = 0} D)
// Every multiply and add is rounded on its own: no fmaf is written here and the unit is built with -ffp-contract=off.
//
// Demappers.  LDPC_DEMAP_MAXLOG is the rule above.  LDPC_DEMAP_EXACT (sym_axis_exact, the EXACT instantiations) adds the
// log-sum-exp correction of include/ldpc_hip.h to it, each set normalised by its own minimum m_b:
//   S_b = sum_{a': b_k = b} expf(-0.5f * (D(a') - m_b)) in ascending level index;  llr_k = 0.5f * (m1 - m0) + (logf(S_0) - logf(S_1))
// For h = 1 both sums are 1.0f and the rule is max-log bit for bit: the host sends m <= 2 to the max-log instantiations.
// sym_demap applies either rule to received samples (vI, vQ, e, 0) that a caller hands in (ldpc_demap_sym).

namespace ldpc {

constexpr uint32_t kSymCounterTag = 0x40000000u;    // third counter word: disjoint from the noise quads (< 2^29 + 256) and the information words (top bit)
constexpr unsigned kSymMaxSymbols = 1u << 29;

// the run of M floats of one symbol at dst, whose address is PH floats past a 16-byte boundary: 16-byte stores where the
// address allows them, then 8-byte ones, else single floats.  Everything is resolved at compile time, so v stays in registers.
template <int M, int PH, int P = 0>
__device__ inline void sym_store_run(float *dst, const float (&v)[M])
{
    if constexpr (P < M) {
        constexpr int ph = (PH + P) & 3;
        if constexpr (ph == 0 && M - P >= 4) {
            *reinterpret_cast<float4 *>(dst + P) = make_float4(v[P], v[P + 1], v[P + 2], v[P + 3]);
            sym_store_run<M, PH, P + 4>(dst, v);
        } else if constexpr ((ph & 1) == 0 && M - P >= 2) {
            *reinterpret_cast<float2 *>(dst + P) = make_float2(v[P], v[P + 1]);
            sym_store_run<M, PH, P + 2>(dst, v);
        } else {
            dst[P] = v[P];
            sym_store_run<M, PH, P + 1>(dst, v);
        }
    }
}

// a lane's M consecutive LLRs: the widest stores its address allows (a row starts at byte 4 * b * n and a symbol M floats on, so
// every alignment occurs); the last symbol of a row stores its cnt < M live values one by one
template <int M>
__device__ inline void sym_store(float *dst, const float (&v)[M], int cnt)
{
    if (cnt == M) {
        if constexpr (M == 1) {
            dst[0] = v[0];
        } else {
            switch ((unsigned)((uintptr_t)dst >> 2) & 3u) {
            case 0: sym_store_run<M, 0>(dst, v); break;
            case 1: sym_store_run<M, 1>(dst, v); break;
            case 2: sym_store_run<M, 2>(dst, v); break;
            default: sym_store_run<M, 3>(dst, v); break;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < M; ++k)
            if (k < cnt) dst[k] = v[k];
    }
}

// the lane's (frame, symbol): one lane per symbol, consecutive lanes hold consecutive symbols of the [batch][S] block -- the
// lane-to-(frame, symbol) arithmetic of sim_channel_awgn.  b may lie past the block: the caller returns then.
__device__ inline void sym_lane(unsigned S, long long &b, unsigned &s)
{
    const unsigned long long g0 = (unsigned long long)blockIdx.x * kSimBlock;     // first symbol of the workgroup: uniform
    const unsigned long long b0 = g0 / S;
    const unsigned t = (unsigned)(g0 - b0 * S) + threadIdx.x;                     // < S + 256 < 2^29 + 256
    const unsigned db = t / S;
    b = (long long)b0 + db;
    s = t - db * S;
}

// the symbol's bits out of the frame's packed codeword row (NULL: the all-zero word), bit k of the symbol at bit k, pad bits 0.
// Permuted path: p[k] = pos[j0 + k] is the variable of bit k (0 for a pad bit).  Identity path: cnt bits from bit j0 of the row on.
template <int M, bool PERM>
__device__ inline unsigned sym_bits(const uint8_t *row, const int *pos, int j0, int cnt, int rb, int (&p)[M])
{
    unsigned bits = 0;
    if constexpr (PERM) {
#pragma unroll
        for (int k = 0; k < M; ++k) {
            p[k] = k < cnt ? pos[j0 + k] : 0;
            if (row && k < cnt) bits |= ((unsigned)(row[p[k] >> 3] >> (p[k] & 7)) & 1u) << k;
        }
    } else if (row) {
        const int byte = j0 >> 3, sh = j0 & 7;
        unsigned w = row[byte];
        if ((M & (M - 1)) != 0 && byte + 1 < rb) w |= (unsigned)row[byte + 1] << 8;   // M = 3, 5, 6: a run can reach into the next byte
        bits = (w >> sh) & ((1u << cnt) - 1u);
    }
    return bits;
}

// the lane's M values into row dst: the pos[] scatter, or the run of floats j0 .. j0 + cnt - 1
template <int M, bool PERM>
__device__ inline void sym_put(float *dst, const int (&p)[M], int j0, int cnt, const float (&v)[M])
{
    if constexpr (PERM) {
#pragma unroll
        for (int k = 0; k < M; ++k)
            if (k < cnt) dst[p[k]] = v[k];
    } else {
        sym_store<M>(dst + j0, v, cnt);
    }
}

// one axis of H bits: `bits` holds b_k at bit k (b_0, the most significant label bit, at bit 0).  Sends the labelled amplitude
// through v = e * a + z, forms the 2^H squared distances once and takes the H masked minima out of them.
template <int H>
__device__ inline float sym_axis(unsigned bits, float e, float z, float *llr)
{
    constexpr int L = 1 << H;
    unsigned i = 0, run = 0;
#pragma unroll
    for (int k = 0; k < H; ++k) {
        run ^= (bits >> k) & 1u;
        i = (i << 1) | run;
    }
    const int a = (L - 1) - 2 * (int)i;
    const float ea = e * (float)a;
    const float v = ea + z;
    float D[L];
#pragma unroll
    for (int c = 0; c < L; ++c) {
        const float ec = e * (float)((L - 1) - 2 * c);
        const float t = v - ec;
        D[c] = t * t;
    }
#pragma unroll
    for (int k = 0; k < H; ++k) {
        float m0 = INFINITY, m1 = INFINITY;
#pragma unroll
        for (int c = 0; c < L; ++c) {
            const int gray = c ^ (c >> 1);                                        // label of level c, b_0 at bit H - 1
            if ((gray >> (H - 1 - k)) & 1) m1 = fminf(m1, D[c]);
            else m0 = fminf(m0, D[c]);
        }
        const float d = m1 - m0;
        llr[k] = 0.5f * d;
    }
    return v;
}

// the axis of a received sample: sym_axis from v on -- the same 2^H distances in the same operations and the same masked
// minima, so a sample that sim_channel_sym stored demaps to the LLRs that kernel stored, bit for bit
template <int H>
__device__ inline void sym_demap_axis(float v, float e, float *llr)
{
    constexpr int L = 1 << H;
    float D[L];
#pragma unroll
    for (int c = 0; c < L; ++c) {
        const float ec = e * (float)((L - 1) - 2 * c);
        const float t = v - ec;
        D[c] = t * t;
    }
#pragma unroll
    for (int k = 0; k < H; ++k) {
        float m0 = INFINITY, m1 = INFINITY;
#pragma unroll
        for (int c = 0; c < L; ++c) {
            const int gray = c ^ (c >> 1);
            if ((gray >> (H - 1 - k)) & 1) m1 = fminf(m1, D[c]);
            else m0 = fminf(m0, D[c]);
        }
        const float d = m1 - m0;
        llr[k] = 0.5f * d;
    }
}

// the exact (log-MAP) rule on the distances of sym_axis: the max-log LLR plus logf(S_0) - logf(S_1), S_b the sum over the
// levels with b_k = b of expf(-0.5f * (D - m_b)) in ascending level index.  Each set is normalised by its own minimum, so
// 1 <= S_b <= L / 2 and nothing underflows into logf(0).  H * 2^H expf and 2 H logf per axis; D stays in registers (every
// index is a compile-time constant after unrolling).
template <int H>
__device__ inline void sym_demap_axis_exact(float v, float e, float *llr)
{
    constexpr int L = 1 << H;
    float D[L];
#pragma unroll
    for (int c = 0; c < L; ++c) {
        const float ec = e * (float)((L - 1) - 2 * c);
        const float t = v - ec;
        D[c] = t * t;
    }
#pragma unroll
    for (int k = 0; k < H; ++k) {
        float m0 = INFINITY, m1 = INFINITY;
#pragma unroll
        for (int c = 0; c < L; ++c) {
            const int gray = c ^ (c >> 1);                                        // label of level c, b_0 at bit H - 1
            if ((gray >> (H - 1 - k)) & 1) m1 = fminf(m1, D[c]);
            else m0 = fminf(m0, D[c]);
        }
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int c = 0; c < L; ++c) {
            const int gray = c ^ (c >> 1);
            if ((gray >> (H - 1 - k)) & 1) {
                const float x = D[c] - m1;
                s1 = s1 + expf(-0.5f * x);
            } else {
                const float x = D[c] - m0;
                s0 = s0 + expf(-0.5f * x);
            }
        }
        const float d = m1 - m0;
        const float corr = logf(s0) - logf(s1);
        llr[k] = 0.5f * d + corr;
    }
}

// sym_axis with the exact rule: the same level, the same ea and the same v = ea + z, then sym_demap_axis_exact
template <int H>
__device__ inline float sym_axis_exact(unsigned bits, float e, float z, float *llr)
{
    constexpr int L = 1 << H;
    unsigned i = 0, run = 0;
#pragma unroll
    for (int k = 0; k < H; ++k) {
        run ^= (bits >> k) & 1u;
        i = (i << 1) | run;
    }
    const int a = (L - 1) - 2 * (int)i;
    const float ea = e * (float)a;
    const float v = ea + z;
    sym_demap_axis_exact<H>(v, e, llr);
    return v;
}

// LLRs from received samples (ldpc_demap_sym): one lane per symbol with the lane-to-(frame, symbol) arithmetic of
// sim_channel_sym, one 16-byte load of (vI, vQ, e, 0), the axis rule on (vI, e) and (vQ, e), and that kernel's stores: the
// lane's M floats of row b, or the pos[] scatter.  256-thread workgroups, no LDS, no random numbers; pad bits are not stored.
template <int M, bool PERM, bool EXACT>
__global__ __launch_bounds__(kSimBlock) void sym_demap(float *__restrict__ llr, long long batch, int n, unsigned S,
                                                       const int *__restrict__ pos, const float4 *__restrict__ received)
{
    constexpr int H = M == 1 ? 1 : M / 2;
    long long b;
    unsigned s;
    sym_lane(S, b, s);
    if (b >= batch) return;
    const int j0 = (int)s * M;                                                    // < n <= 2^31 - 1
    const int cnt = n - j0 < M ? n - j0 : M;
    const float4 r = received[(size_t)b * S + s];
    float v[M];
    if constexpr (EXACT) {
        sym_demap_axis_exact<H>(r.x, r.z, v);
        if constexpr (M > 1) sym_demap_axis_exact<H>(r.y, r.z, v + H);
    } else {
        sym_demap_axis<H>(r.x, r.z, v);
        if constexpr (M > 1) sym_demap_axis<H>(r.y, r.z, v + H);
    }
    float *dst = llr + (size_t)b * (size_t)n;
    if constexpr (PERM) {
#pragma unroll
        for (int k = 0; k < M; ++k)
            if (k < cnt) dst[pos[j0 + k]] = v[k];
    } else {
        sym_store<M>(dst + j0, v, cnt);
    }
}

// One lane per symbol; consecutive lanes hold consecutive symbols of the [batch][S] block, the lane-to-(frame, symbol)
// arithmetic of sim_channel_awgn.  256-thread workgroups, no LDS.  Identity path (PERM false): the lane owns floats
// s * M .. s * M + M - 1 of row b.  Permuted path: bit k of the symbol is the codeword bit of variable pos[s * M + k], and its
// LLR goes there with a 4-byte store.  cw_stride 0: one codeword for every frame; cw NULL: the all-zero word.
template <int M, bool FADING, bool PERM, bool EXACT>
__global__ __launch_bounds__(kSimBlock) void sim_channel_sym(float *__restrict__ llr, long long batch, int n, unsigned S,
                                                             uint32_t k0, uint32_t k1, uint32_t stream_id,
                                                             unsigned long long first_frame, float amp,
                                                             const int *__restrict__ pos, const uint8_t *__restrict__ cw,
                                                             long long cw_stride, float4 *__restrict__ received)
{
    constexpr int H = M == 1 ? 1 : M / 2;
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
    const unsigned bits = sym_bits<M, PERM>(row, pos, j0, cnt, rb, p);            // bit k of the symbol at bit k; pad bits 0
    const unsigned long long f = first_frame + (unsigned long long)b;
    uint32_t x[4];
    philox4x32_10((uint32_t)f, (uint32_t)(f >> 32), kSymCounterTag | s, stream_id, k0, k1, x);
    float zI, zQ;
    sim_box_muller(x[0], x[1], zI, zQ);
    float g = 1.0f;
    if (FADING) g = sqrtf(-logf(sim_uniform(x[2])));
    const float e = g * amp;
    float v[M];
    float vI, vQ = 0.0f;
    if constexpr (EXACT) {
        vI = sym_axis_exact<H>(bits & ((1u << H) - 1u), e, zI, v);
        if constexpr (M > 1) vQ = sym_axis_exact<H>(bits >> H, e, zQ, v + H);
    } else {
        vI = sym_axis<H>(bits & ((1u << H) - 1u), e, zI, v);
        if constexpr (M > 1) vQ = sym_axis<H>(bits >> H, e, zQ, v + H);
    }
    if (received) received[(size_t)b * S + s] = make_float4(vI, vQ, e, 0.0f);
    float *dst = llr + (size_t)b * (size_t)n;
    sym_put<M, PERM>(dst, p, j0, cnt, v);
}

// sim_channel_sym with the SNR point a function of the frame and the sent bits as training targets (ldpc_channel_sym_mix):
// amp = amp_tab[p], p = f mod K of the absolute frame index f = first_frame + b, the remainder taken as sim_channel_awgn_mix
// takes it (p0 = first_frame mod K and Kinv = floor((2^32 - 1) / K) from the host, b <= 2^31 - 1 and K <= 4096 keep
// r = b + p0 below 2^32, umulhi and one conditional subtraction).  The table read is issued before the Philox rounds and
// hidden behind them; a wave covers 64 / S + 1 rows at most, so it is nearly wave-uniform, and 4096 floats stay in cache.
// The lane-per-symbol mapping, the counters, the normals, the fading gain, sym_axis and the stores are sim_channel_sym's,
// which is left as it is: a frame gets what that kernel gives it at amp = amp_tab[p], bit for bit.  targets, when not NULL,
// receives the symbol's bits as 0.0f / 1.0f where the LLRs go: the lane holds them in `bits` already.  The two rows start at
// unrelated addresses, so each output picks its store widths from its own address; pad bits are stored in neither.
template <int M, bool FADING, bool PERM, bool EXACT>
__global__ __launch_bounds__(kSimBlock) void sim_channel_sym_mix(float *__restrict__ llr, float *__restrict__ targets,
                                                                 long long batch, int n, unsigned S, uint32_t k0, uint32_t k1,
                                                                 uint32_t stream_id, unsigned long long first_frame,
                                                                 unsigned p0, unsigned K, unsigned Kinv,
                                                                 const float *__restrict__ amp_tab,
                                                                 const int *__restrict__ pos, const uint8_t *__restrict__ cw,
                                                                 long long cw_stride)
{
    constexpr int H = M == 1 ? 1 : M / 2;
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
    const unsigned bits = sym_bits<M, PERM>(row, pos, j0, cnt, rb, p);            // bit k of the symbol at bit k; pad bits 0
    const unsigned long long f = first_frame + (unsigned long long)b;
    uint32_t x[4];
    philox4x32_10((uint32_t)f, (uint32_t)(f >> 32), kSymCounterTag | s, stream_id, k0, k1, x);
    float zI, zQ;
    sim_box_muller(x[0], x[1], zI, zQ);
    float g = 1.0f;
    if (FADING) g = sqrtf(-logf(sim_uniform(x[2])));
    const float e = g * amp;
    float v[M];
    if constexpr (EXACT) {
        sym_axis_exact<H>(bits & ((1u << H) - 1u), e, zI, v);
        if constexpr (M > 1) sym_axis_exact<H>(bits >> H, e, zQ, v + H);
    } else {
        sym_axis<H>(bits & ((1u << H) - 1u), e, zI, v);
        if constexpr (M > 1) sym_axis<H>(bits >> H, e, zQ, v + H);
    }
    float *dst = llr + (size_t)b * (size_t)n;
    if constexpr (PERM) {                                                         // sym_put, written out: through the helper the
#pragma unroll                                                                    // permuted exact forms take two more VGPRs
        for (int k = 0; k < M; ++k)
            if (k < cnt) dst[p[k]] = v[k];
    } else {
        sym_store<M>(dst + j0, v, cnt);
    }
    if (targets) {
        float sent[M];
#pragma unroll
        for (int k = 0; k < M; ++k) sent[k] = ((bits >> k) & 1u) ? 1.0f : 0.0f;
        float *tdst = targets + (size_t)b * (size_t)n;
        if constexpr (PERM) {
#pragma unroll
            for (int k = 0; k < M; ++k)
                if (k < cnt) tdst[p[k]] = sent[k];
        } else {
            sym_store<M>(tdst + j0, sent, cnt);
        }
    }
}

}  // namespace ldpc

namespace {

// the scalar part of a modulation descriptor (the position table is a device pointer: the caller vouches for it); the mix
// entry reads its amplitudes from a device table and passes check_amp = false; ldpc_demap_sym reads the gain out of the
// samples and ignores fading as well
int sym_mod_check(const ldpc_modulation *mod, int32_t n, bool check_amp = true, bool check_fading = true)
{
    if (!mod) return fail(LDPC_ERR_ARG, "NULL mod");
    const int32_t m = mod->bits_per_symbol;
    if (m != 1 && m != 2 && m != 4 && m != 6 && m != 8)
        return fail(LDPC_ERR_ARG, "bits_per_symbol must be 1, 2, 4, 6 or 8 (BPSK, QPSK, 16- / 64- / 256-QAM), got %d", m);
    if (check_fading && mod->fading != 0 && mod->fading != 1)
        return fail(LDPC_ERR_ARG, "fading must be 0 (none) or 1 (Rayleigh per symbol), got %d", mod->fading);
    if (check_amp && !(std::isfinite(mod->amp) && mod->amp >= 0.0f)) return fail(LDPC_ERR_ARG, "amp must be finite and >= 0");
    if (((int64_t)n + m - 1) / m >= (int64_t)kSymMaxSymbols)
        return fail(LDPC_ERR_UNSUPPORTED, "a frame of %lld symbols: the symbol index must stay below 2^29", (long long)(((int64_t)n + m - 1) / m));
    return LDPC_OK;
}

int sym_demapper_check(int32_t demapper)
{
    if (demapper != LDPC_DEMAP_MAXLOG && demapper != LDPC_DEMAP_EXACT)
        return fail(LDPC_ERR_ARG, "demapper must be LDPC_DEMAP_MAXLOG (0) or LDPC_DEMAP_EXACT (1), got %d", demapper);
    return LDPC_OK;
}

// the EXACT instantiations exist for m >= 4 only: one bit per axis has one level per set, both sums are 1.0f and the exact
// rule is the max-log rule bit for bit
inline bool sym_exact(int32_t demapper, int m) { return demapper == LDPC_DEMAP_EXACT && m >= 4; }

template <int M, bool FADING, bool EXACT>
void sym_launch_perm(bool perm, dim3 grid, hipStream_t s, float *llr, long long batch, int n, unsigned S, uint32_t k0, uint32_t k1,
                     uint32_t stream_id, unsigned long long first_frame, float amp, const int *pos, const uint8_t *cw,
                     long long cw_stride, float4 *received)
{
    if (perm)
        hipLaunchKernelGGL((sim_channel_sym<M, FADING, true, EXACT>), grid, dim3(kSimBlock), 0, s, llr, batch, n, S, k0, k1, stream_id,
                           first_frame, amp, pos, cw, cw_stride, received);
    else
        hipLaunchKernelGGL((sim_channel_sym<M, FADING, false, EXACT>), grid, dim3(kSimBlock), 0, s, llr, batch, n, S, k0, k1, stream_id,
                           first_frame, amp, pos, cw, cw_stride, received);
}

// one launch of sim_channel_sym; mod has passed sym_mod_check and demapper sym_demapper_check
int sim_channel_sym_launch(float *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                           const ldpc_modulation *mod, int32_t demapper, const uint8_t *cw, int64_t cw_stride, void *received,
                           hipStream_t s)
{
    const int m = mod->bits_per_symbol;
    const unsigned S = (unsigned)(((int64_t)n + m - 1) / m);
    const unsigned long long syms = (unsigned long long)batch * S;
    const unsigned long long blocks = (syms + kSimBlock - 1) / kSimBlock;
    if (blocks > 0x7fffffffull) return fail(LDPC_ERR_UNSUPPORTED, "batch too large for one launch");
    const dim3 grid((unsigned)blocks);
    const bool perm = mod->position != nullptr, fading = mod->fading != 0;
#define LDPC_SYM_ARGS                                                                                                             \
    perm, grid, s, llr, (long long)batch, (int)n, S, (uint32_t)seed, (uint32_t)(seed >> 32), stream_id,                           \
        (unsigned long long)first_frame, mod->amp, (const int *)mod->position, cw, (long long)cw_stride, (float4 *)received
#define LDPC_SYM_CASE(M, EXACT)                                                                                                   \
    case M:                                                                                                                       \
        if (fading) sym_launch_perm<M, true, EXACT>(LDPC_SYM_ARGS);                                                               \
        else sym_launch_perm<M, false, EXACT>(LDPC_SYM_ARGS);                                                                     \
        break;
    if (sym_exact(demapper, m)) {
        switch (m) {
            LDPC_SYM_CASE(4, true)
            LDPC_SYM_CASE(6, true)
            LDPC_SYM_CASE(8, true)
        default: return fail(LDPC_ERR_ARG, "bits_per_symbol %d", m);
        }
    } else {
        switch (m) {
            LDPC_SYM_CASE(1, false)
            LDPC_SYM_CASE(2, false)
            LDPC_SYM_CASE(4, false)
            LDPC_SYM_CASE(6, false)
            LDPC_SYM_CASE(8, false)
        default: return fail(LDPC_ERR_ARG, "bits_per_symbol %d", m);
        }
    }
#undef LDPC_SYM_CASE
#undef LDPC_SYM_ARGS
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

struct SymMixArgs {
    float *llr, *targets;
    long long batch;
    int n;
    unsigned S;
    uint32_t k0, k1, stream_id;
    unsigned long long first_frame;
    unsigned p0, K, Kinv;
    const float *amp_tab;
    const int *pos;
    const uint8_t *cw;
    long long cw_stride;
};

template <int M, bool FADING, bool PERM, bool EXACT>
void sym_mix_launch_one(dim3 grid, hipStream_t s, const SymMixArgs &a)
{
    hipLaunchKernelGGL((sim_channel_sym_mix<M, FADING, PERM, EXACT>), grid, dim3(kSimBlock), 0, s, a.llr, a.targets, a.batch, a.n, a.S,
                       a.k0, a.k1, a.stream_id, a.first_frame, a.p0, a.K, a.Kinv, a.amp_tab, a.pos, a.cw, a.cw_stride);
}

template <int M, bool EXACT>
void sym_mix_launch_m(bool fading, bool perm, dim3 grid, hipStream_t s, const SymMixArgs &a)
{
    if (fading) {
        if (perm) sym_mix_launch_one<M, true, true, EXACT>(grid, s, a);
        else sym_mix_launch_one<M, true, false, EXACT>(grid, s, a);
    } else {
        if (perm) sym_mix_launch_one<M, false, true, EXACT>(grid, s, a);
        else sym_mix_launch_one<M, false, false, EXACT>(grid, s, a);
    }
}

// one launch of sim_channel_sym_mix; mod has passed sym_mod_check, demapper sym_demapper_check, 1 <= n_points <= 4096 and
// batch <= 2^31 - 1
int sim_channel_sym_mix_launch(float *llr, float *targets, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id,
                               uint64_t first_frame, const ldpc_modulation *mod, int32_t demapper, const float *amp_tab,
                               int32_t n_points, const uint8_t *cw, int64_t cw_stride, hipStream_t s)
{
    const int m = mod->bits_per_symbol;
    const unsigned S = (unsigned)(((int64_t)n + m - 1) / m);
    const unsigned long long syms = (unsigned long long)batch * S;
    const unsigned long long blocks = (syms + kSimBlock - 1) / kSimBlock;
    if (blocks > 0x7fffffffull) return fail(LDPC_ERR_UNSUPPORTED, "batch too large for one launch");
    const dim3 grid((unsigned)blocks);
    const bool perm = mod->position != nullptr, fading = mod->fading != 0;
    const unsigned K = (unsigned)n_points;
    const SymMixArgs a{llr, targets, (long long)batch, (int)n, S, (uint32_t)seed, (uint32_t)(seed >> 32), stream_id,
                       (unsigned long long)first_frame, (unsigned)(first_frame % K), K, 0xffffffffu / K, amp_tab,
                       (const int *)mod->position, cw, (long long)cw_stride};
    if (sym_exact(demapper, m)) {
        switch (m) {
        case 4: sym_mix_launch_m<4, true>(fading, perm, grid, s, a); break;
        case 6: sym_mix_launch_m<6, true>(fading, perm, grid, s, a); break;
        case 8: sym_mix_launch_m<8, true>(fading, perm, grid, s, a); break;
        default: return fail(LDPC_ERR_ARG, "bits_per_symbol %d", m);
        }
    } else {
        switch (m) {
        case 1: sym_mix_launch_m<1, false>(fading, perm, grid, s, a); break;
        case 2: sym_mix_launch_m<2, false>(fading, perm, grid, s, a); break;
        case 4: sym_mix_launch_m<4, false>(fading, perm, grid, s, a); break;
        case 6: sym_mix_launch_m<6, false>(fading, perm, grid, s, a); break;
        case 8: sym_mix_launch_m<8, false>(fading, perm, grid, s, a); break;
        default: return fail(LDPC_ERR_ARG, "bits_per_symbol %d", m);
        }
    }
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

template <int M, bool EXACT>
void sym_demap_launch_one(bool perm, dim3 grid, hipStream_t s, float *llr, long long batch, int n, unsigned S, const int *pos,
                          const float4 *received)
{
    if (perm) hipLaunchKernelGGL((sym_demap<M, true, EXACT>), grid, dim3(kSimBlock), 0, s, llr, batch, n, S, pos, received);
    else hipLaunchKernelGGL((sym_demap<M, false, EXACT>), grid, dim3(kSimBlock), 0, s, llr, batch, n, S, pos, received);
}

// one launch of sym_demap; mod has passed sym_mod_check and demapper sym_demapper_check
int sym_demap_launch(float *llr, int64_t batch, int32_t n, const ldpc_modulation *mod, int32_t demapper, const void *received,
                     hipStream_t s)
{
    const int m = mod->bits_per_symbol;
    const unsigned S = (unsigned)(((int64_t)n + m - 1) / m);
    const unsigned long long syms = (unsigned long long)batch * S;
    const unsigned long long blocks = (syms + kSimBlock - 1) / kSimBlock;
    if (blocks > 0x7fffffffull) return fail(LDPC_ERR_UNSUPPORTED, "batch too large for one launch");
    const dim3 grid((unsigned)blocks);
    const bool perm = mod->position != nullptr;
    const int *pos = (const int *)mod->position;
    const float4 *rec = (const float4 *)received;
    if (sym_exact(demapper, m)) {
        switch (m) {
        case 4: sym_demap_launch_one<4, true>(perm, grid, s, llr, (long long)batch, (int)n, S, pos, rec); break;
        case 6: sym_demap_launch_one<6, true>(perm, grid, s, llr, (long long)batch, (int)n, S, pos, rec); break;
        case 8: sym_demap_launch_one<8, true>(perm, grid, s, llr, (long long)batch, (int)n, S, pos, rec); break;
        default: return fail(LDPC_ERR_ARG, "bits_per_symbol %d", m);
        }
    } else {
        switch (m) {
        case 1: sym_demap_launch_one<1, false>(perm, grid, s, llr, (long long)batch, (int)n, S, pos, rec); break;
        case 2: sym_demap_launch_one<2, false>(perm, grid, s, llr, (long long)batch, (int)n, S, pos, rec); break;
        case 4: sym_demap_launch_one<4, false>(perm, grid, s, llr, (long long)batch, (int)n, S, pos, rec); break;
        case 6: sym_demap_launch_one<6, false>(perm, grid, s, llr, (long long)batch, (int)n, S, pos, rec); break;
        case 8: sym_demap_launch_one<8, false>(perm, grid, s, llr, (long long)batch, (int)n, S, pos, rec); break;
        default: return fail(LDPC_ERR_ARG, "bits_per_symbol %d", m);
        }
    }
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

// simulate_enc_impl's loop with the symbol channel: encode_random (or the descriptor's one codeword), sim_channel_sym,
// ldpc_decode, the decisions XORed with the codeword rows (one codeword: the counters compare against it themselves), the
// existing counters.  The channel is a parameter (ldpc_simulate_con runs the same loop on a constellation table):
// check(n) validates its descriptor where sym_mod_check / sym_demapper_check stand, channel(llr, frames, first, cw, stride, s)
// is the one launch of a block.
template <class Check, class Channel>
int simulate_symbols_impl(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_encoder *e, const char *what, Check check,
                          Channel channel, int64_t capture, int64_t out_state[8], int64_t *out_diag, void *workspace,
                          size_t workspace_bytes, void *stream)
{
    const bool diagnostics = capture >= 0;
    if (!d || !desc || !out_state) return fail(LDPC_ERR_ARG, "NULL decoder / descriptor / out_state");
    if (diagnostics && !out_diag) return fail(LDPC_ERR_ARG, "NULL out_diag");
    if (diagnostics && sim_diag_words(d->T, capture) == 0) return fail(LDPC_ERR_ARG, "capture too large");
    if (e && desc->codeword_packed) return fail(LDPC_ERR_ARG, "codeword_packed must be NULL with an encoder: the codewords are drawn per frame");
    if (desc->block < 1) return fail(LDPC_ERR_ARG, "block < 1");
    if (desc->poll_blocks < 1) return fail(LDPC_ERR_ARG, "poll_blocks < 1");
    if (d->dtype != LDPC_F32) return fail(LDPC_ERR_UNSUPPORTED, "%s draws fp32 LLRs: float64 decoders are not supported", what);
    if (d->g->n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (int rc = check(d->g->n)) return rc;
    if (e && e->g.n != d->g->n) return fail(LDPC_ERR_ARG, "the encoder has n = %d, the decoder n = %d", e->g.n, d->g->n);
    if (e && e->device != d->g->device) return fail(LDPC_ERR_ARG, "encoder and decoder live on different devices");
    if (!workspace) return fail(LDPC_ERR_ARG, "NULL workspace");
    if (((uintptr_t)workspace % kAlign) != 0) return fail(LDPC_ERR_ARG, "workspace must be %zu-byte aligned", kAlign);
    const SimWorkspace w = sim_carve(d, desc->block, capture);
    const size_t total = sim_enc_total(d, desc->block, capture);
    if (total > workspace_bytes) return fail(LDPC_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, total);
    DeviceGuard guard(d->g->device);
    hipStream_t s = (hipStream_t)stream;
    char *base = (char *)workspace;
    float *llr = (float *)(base + w.o_llr);
    uint8_t *packed = (uint8_t *)(base + w.o_packed);
    int32_t *iters = (int32_t *)(base + w.o_iters);
    int64_t *state = (int64_t *)(base + w.o_state);
    uint8_t *success = diagnostics ? (uint8_t *)(base + w.o_success) : nullptr;
    uint32_t *words = diagnostics ? (uint32_t *)(base + w.o_words) : nullptr;
    int64_t *diag = diagnostics ? (int64_t *)(base + w.o_diag) : nullptr;
    uint8_t *cw = (uint8_t *)(base + sim_enc_cw_offset(d, desc->block, capture));
    const int32_t n = d->g->n;
    const long long rb = ((long long)n + 7) / 8;
    const uint8_t *one = e ? nullptr : desc->codeword_packed;       // the counters' codeword: rows are XORed away instead
    PinnedState host;
    HIP_TRY(hipHostMalloc((void **)&host.p, 8 * sizeof(int64_t), hipHostMallocDefault));
    HIP_TRY(hipMemsetAsync(state, 0, 8 * sizeof(int64_t), s));
    if (diagnostics) HIP_TRY(hipMemsetAsync(diag, 0, w.diag_words * sizeof(int64_t), s));
    auto count = [&](int64_t frames, int64_t first) {    // fold one block (frames = 0: latch `done`)
        if (diagnostics)
            return sim_count_diag_launch(state, diag, d->T, capture, packed, iters, success, frames, n, one,
                                         desc->first_frame + (uint64_t)first, desc->max_frames, desc->max_errors, words, s);
        return sim_count_launch(state, packed, iters, frames, n, one, desc->max_frames, desc->max_errors, s);
    };
    int64_t drawn = 0;                                   // frames drawn so far: block k starts at first_frame + k * block
    for (;;) {
        int queued = 0;
        for (int p = 0; p < desc->poll_blocks && drawn < desc->max_frames; ++p, ++queued) {
            const int64_t frames = std::min<int64_t>(desc->block, desc->max_frames - drawn);
            const uint64_t first = desc->first_frame + (uint64_t)drawn;
            if (e)
                if (int rc = enc_launch(e, frames, 1, desc->seed, desc->stream_id, first, nullptr, cw, nullptr, s)) return rc;
            if (int rc = channel(llr, frames, first, e ? (const uint8_t *)cw : one, e ? rb : 0, s)) return rc;
            if (int rc = ldpc_decode(d, llr, frames, 1, nullptr, nullptr, iters, success, packed, base + w.o_dec, w.dec_bytes, s))
                return rc;
            if (e) {
                const long long bytes = (long long)frames * rb, xblocks = ((bytes >> 2) + kSimBlock - 1) / kSimBlock;
                hipLaunchKernelGGL(enc_xor_rows, dim3((unsigned)std::max<long long>(xblocks, 1)), dim3(kSimBlock), 0, s, packed,
                                   (const uint8_t *)cw, bytes);
                HIP_TRY(hipGetLastError());
            }
            if (int rc = count(frames, drawn)) return rc;
            drawn += frames;
        }
        if (queued == 0)                                 // max_frames <= 0, or every frame drawn: an empty block latches `done`
            if (int rc = count(0, drawn)) return rc;
        HIP_TRY(hipMemcpyAsync(host.p, state, 8 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (host.p[4] != 0) break;
        if (queued == 0) return fail(LDPC_ERR_HIP, "internal error: every frame counted and the point is not done");
    }
    if (diagnostics) {
        HIP_TRY(hipMemcpyAsync(out_diag, diag, w.diag_words * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (int k = 0; k < 8; ++k) out_state[k] = host.p[k];
    return LDPC_OK;
}

int simulate_sym_impl(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_encoder *e, const ldpc_modulation *mod,
                      int32_t demapper, int64_t capture, int64_t out_state[8], int64_t *out_diag, void *workspace, size_t workspace_bytes,
                      void *stream)
{
    return simulate_symbols_impl(
        d, desc, e, "ldpc_simulate_sym",
        [&](int32_t n) {
            if (int rc = sym_mod_check(mod, n)) return rc;
            return sym_demapper_check(demapper);
        },
        [&](float *llr, int64_t frames, uint64_t first, const uint8_t *cw, int64_t stride, hipStream_t s) {
            return sim_channel_sym_launch(llr, frames, d->g->n, desc->seed, desc->stream_id, first, mod, demapper, cw, stride, nullptr, s);
        },
        capture, out_state, out_diag, workspace, workspace_bytes, stream);
}

}  // namespace

extern "C" {

int ldpc_channel_sym_dm(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                        const ldpc_modulation *mod, const uint8_t *codewords_packed, int64_t codeword_stride, void *received,
                        int32_t demapper, void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (int rc = sym_mod_check(mod, n)) return rc;
    if (int rc = sym_demapper_check(demapper)) return rc;
    if (codeword_stride != 0 && codeword_stride != ((int64_t)n + 7) / 8)
        return fail(LDPC_ERR_ARG, "codeword_stride must be 0 (one codeword) or ceil(n / 8) = %lld (one packed row per frame)",
                    (long long)(((int64_t)n + 7) / 8));
    if (batch == 0) return LDPC_OK;
    if (!llr) return fail(LDPC_ERR_ARG, "NULL llr");
    if (((uintptr_t)llr % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "llr must be 4-byte aligned");
    if (received && ((uintptr_t)received % 16) != 0) return fail(LDPC_ERR_ARG, "received must be 16-byte aligned");
    return sim_channel_sym_launch((float *)llr, batch, n, seed, stream_id, first_frame, mod, demapper, codewords_packed,
                                  codeword_stride, received, (hipStream_t)stream);
}

int ldpc_channel_sym(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                     const ldpc_modulation *mod, const uint8_t *codewords_packed, int64_t codeword_stride, void *received,
                     void *stream)
{
    return ldpc_channel_sym_dm(llr, batch, n, seed, stream_id, first_frame, mod, codewords_packed, codeword_stride, received,
                               LDPC_DEMAP_MAXLOG, stream);
}

int ldpc_demap_sym(void *llr, int64_t batch, int32_t n, const ldpc_modulation *mod, int32_t demapper, const void *received,
                   void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (int rc = sym_mod_check(mod, n, false, false)) return rc;
    if (int rc = sym_demapper_check(demapper)) return rc;
    if (batch == 0) return LDPC_OK;
    if (!llr) return fail(LDPC_ERR_ARG, "NULL llr");
    if (((uintptr_t)llr % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "llr must be 4-byte aligned");
    if (!received) return fail(LDPC_ERR_ARG, "NULL received");
    if (((uintptr_t)received % 16) != 0) return fail(LDPC_ERR_ARG, "received must be 16-byte aligned");
    return sym_demap_launch((float *)llr, batch, n, mod, demapper, received, (hipStream_t)stream);
}

int ldpc_channel_sym_mix_dm(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                            const ldpc_modulation *mod, const float *amp_tab, int32_t n_points,
                            const uint8_t *codewords_packed, int64_t codeword_stride, void *targets, int32_t demapper,
                            void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (int rc = sym_mod_check(mod, n, false)) return rc;
    if (int rc = sym_demapper_check(demapper)) return rc;
    if (codeword_stride != 0 && codeword_stride != ((int64_t)n + 7) / 8)
        return fail(LDPC_ERR_ARG, "codeword_stride must be 0 (one codeword) or ceil(n / 8) = %lld (one packed row per frame)",
                    (long long)(((int64_t)n + 7) / 8));
    if (n_points < 1 || n_points > 4096) return fail(LDPC_ERR_ARG, "n_points must be in 1 .. 4096");
    if (batch > INT32_MAX) return fail(LDPC_ERR_ARG, "batch > 2^31 - 1");
    if (batch > 0 && first_frame > (uint64_t)0 - (uint64_t)batch)       // 2^64 - batch: p is not continuous across the wrap
        return fail(LDPC_ERR_ARG, "first_frame + batch wraps the 64-bit frame index");
    if (batch > 0 && !amp_tab) return fail(LDPC_ERR_ARG, "NULL amp_tab");
    if (batch == 0) return LDPC_OK;
    if (!llr) return fail(LDPC_ERR_ARG, "NULL llr");
    if (((uintptr_t)llr % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "llr must be 4-byte aligned");
    if (targets && ((uintptr_t)targets % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "targets must be 4-byte aligned");
    if (((uintptr_t)amp_tab % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "amp_tab must be 4-byte aligned");
    return sim_channel_sym_mix_launch((float *)llr, (float *)targets, batch, n, seed, stream_id, first_frame, mod, demapper,
                                      amp_tab, n_points, codewords_packed, codeword_stride, (hipStream_t)stream);
}

int ldpc_channel_sym_mix(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                         const ldpc_modulation *mod, const float *amp_tab, int32_t n_points, const uint8_t *codewords_packed,
                         int64_t codeword_stride, void *targets, void *stream)
{
    return ldpc_channel_sym_mix_dm(llr, batch, n, seed, stream_id, first_frame, mod, amp_tab, n_points, codewords_packed,
                                   codeword_stride, targets, LDPC_DEMAP_MAXLOG, stream);
}

size_t ldpc_simulate_sym_workspace_bytes(const ldpc_decoder *d, int64_t block, int64_t capture)
{
    return ldpc_simulate_enc_workspace_bytes(d, block, capture);
}

int ldpc_simulate_sym_dm(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_encoder *e, const ldpc_modulation *mod,
                         int32_t demapper, int64_t capture, int64_t out_state[8], int64_t *out_diag, void *workspace,
                         size_t workspace_bytes, void *stream)
{
    LDPC_NOTHROW(simulate_sym_impl(d, desc, e, mod, demapper, capture < 0 ? -1 : capture, out_state, out_diag, workspace,
                                   workspace_bytes, stream))
}

int ldpc_simulate_sym(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_encoder *e, const ldpc_modulation *mod,
                      int64_t capture, int64_t out_state[8], int64_t *out_diag, void *workspace, size_t workspace_bytes,
                      void *stream)
{
    return ldpc_simulate_sym_dm(d, desc, e, mod, LDPC_DEMAP_MAXLOG, capture, out_state, out_diag, workspace, workspace_bytes,
                                stream);
}

}  // extern "C"
