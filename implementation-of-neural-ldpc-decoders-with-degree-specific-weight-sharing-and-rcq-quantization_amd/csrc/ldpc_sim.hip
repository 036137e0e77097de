// ldpc_sim.hip -- on-device Monte-Carlo: counter-based AWGN channel, error counters with the reference's in-order stop rule,
// and the host loop of one SNR point (ldpc_channel_awgn / ldpc_sim_count / ldpc_simulate of include/ldpc_hip.h).
//
// Included by ldpc_hip.hip below the decode entry points (it calls ldpc_decode and uses that file's fail / HIP_TRY /
// align_up / DeviceGuard): still the one compiled unit.
//
// Stream definition ("Noise stream"; tests/philox_reference.py restates it in numpy).  Sample j of frame f:
//   (x0, x1, x2, x3) = Philox4x32-10(counter = (f & 0xffffffff, f >> 32, j / 4, stream_id), key = (seed & 0xffffffff, seed >> 32))
//   u(x) = fmaf((float)x, 0x1p-32f, 0x1p-33f)                      in (0, 1], uint -> float rounds to nearest
//   r = sqrtf(-2.0f * logf(u(x0))),  theta = 6.2831853071795865f * u(x1),  z[4q] = r * cosf(theta),  z[4q+1] = r * sinf(theta)
//   (x2, x3) give z[4q+2], z[4q+3] the same way;  llr = s_j * fmaf(z, scale, shift),  s_j = +1 / -1 for codeword bit 0 / 1.
// The smallest uniform is 2^-33, so |z| <= sqrt(66 ln 2) = 6.76: the tails of the normal are cut at +-6.76 sigma.
// The unit is built without fast-math and with -ffp-contract=off: logf / sincosf / sqrtf are the accurate ones and a fused
// multiply-add happens exactly where fmaf is written.

namespace ldpc {

constexpr int kSimBlock = 256;          // channel and per-frame count kernels: 4 waves
constexpr int kSimFoldBlock = 1024;     // the single-workgroup fold: 16 waves, one frame per thread and step

__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ inline float sim_uniform(uint32_t x) { return fmaf((float)x, 0x1p-32f, 0x1p-33f); }

__device__ inline void sim_box_muller(uint32_t a, uint32_t b, float &z0, float &z1)
{
    const float r = sqrtf(-2.0f * logf(sim_uniform(a)));
    const float theta = 6.2831853071795865f * sim_uniform(b);
    float sn, cs;
    sincosf(theta, &sn, &cs);
    z0 = r * cs;
    z1 = r * sn;
}

// One lane per quad of four samples; consecutive lanes hold consecutive quads of the [batch][n] block, so a wave's stores
// are one contiguous 1 KiB run wherever rows are whole quads.  A row starts at byte 4 * b * n: 16-byte aligned for every b
// only when n % 4 == 0, 8-byte aligned when n is even, else 4.  The store width is chosen per lane from the address itself
// (one 16-byte store, two 8-byte stores or four 4-byte ones), so any n and any 4-byte aligned base are correct; the tail
// quad of a row stores its n - 4q samples one by one.  The kernel is bound by the Philox rounds and the two accurate
// log / sincos pairs per quad, not by the stores: 256-thread workgroups without LDS leave the wave slots to the compiler's
// register count.
__global__ __launch_bounds__(kSimBlock) void sim_channel_awgn(float *__restrict__ llr, long long batch, int n, unsigned Q,
                                                              uint32_t k0, uint32_t k1, uint32_t stream_id,
                                                              unsigned long long first_frame, float scale, float shift,
                                                              const uint8_t *__restrict__ cw)
{
    const unsigned long long g0 = (unsigned long long)blockIdx.x * kSimBlock;     // first quad of the workgroup: uniform
    const unsigned long long b0 = g0 / Q;
    const unsigned t = (unsigned)(g0 - b0 * Q) + threadIdx.x;                     // < Q + 256 <= 2^29 + 256
    const unsigned db = t / Q;
    const long long b = (long long)b0 + db;
    const unsigned q = t - db * Q;
    if (b >= batch) return;
    const unsigned long long f = first_frame + (unsigned long long)b;
    uint32_t x[4];
    philox4x32_10((uint32_t)f, (uint32_t)(f >> 32), q, stream_id, k0, k1, x);
    float z[4];
    sim_box_muller(x[0], x[1], z[0], z[1]);
    sim_box_muller(x[2], x[3], z[2], z[3]);
    const int j0 = (int)(q * 4u);
    const int cnt = n - j0 < 4 ? n - j0 : 4;
    unsigned cbits = 0;                                                           // codeword bits j0 .. j0+3
    if (cw) cbits = (cw[j0 >> 3] >> (j0 & 7)) & 0xfu;                             // j0 % 8 is 0 or 4: one byte holds all four
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float y = fmaf(z[k], scale, shift);
        v[k] = ((cbits >> k) & 1u) ? -y : y;
    }
    float *dst = llr + (size_t)b * (size_t)n + (size_t)j0;
    if (cnt == 4) {
        const uintptr_t a = (uintptr_t)dst;
        if ((a & 15) == 0) {
            *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        } else if ((a & 7) == 0) {
            *reinterpret_cast<float2 *>(dst) = make_float2(v[0], v[1]);
            *reinterpret_cast<float2 *>(dst + 2) = make_float2(v[2], v[3]);
        } else {
            dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
        }
    } else {
        for (int k = 0; k < cnt; ++k) dst[k] = v[k];
    }
}

// the quad's stores of sim_channel_awgn_mix: the width chosen per lane from the address, as sim_channel_awgn does inline
__device__ inline void sim_store_quad(float *dst, const float v[4], int cnt)
{
    if (cnt == 4) {
        const uintptr_t a = (uintptr_t)dst;
        if ((a & 15) == 0) {
            *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        } else if ((a & 7) == 0) {
            *reinterpret_cast<float2 *>(dst) = make_float2(v[0], v[1]);
            *reinterpret_cast<float2 *>(dst + 2) = make_float2(v[2], v[3]);
        } else {
            dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
        }
    } else {
        for (int k = 0; k < cnt; ++k) dst[k] = v[k];
    }
}

// sim_channel_awgn with the SNR point a function of the frame: (scale, shift) = (scale_tab[p], shift_tab[p]), p = f mod K of
// the absolute frame index f = first_frame + b (ldpc_channel_awgn_mix).  The same lane-per-quad shape, counters, normals and
// stores; sim_channel_awgn itself is left as it is.  The host passes p0 = first_frame mod K, so that the one 64-bit remainder of
// a launch is taken there: b <= 2^31 - 1 and p0 < K <= 4096 keep r = b + p0 below 2^32 and the lane's remainder in 32 bits, and
// that remainder costs no division either: with Kinv = floor((2^32 - 1) / K), also from the host, 2^32 / K - 1 <= Kinv <= 2^32 / K,
// so umulhi(r, Kinv) is floor(r / K) or one less and r - umulhi(r, Kinv) * K lies in [0, 2K): one conditional subtraction.  The
// two table reads are issued before the Philox rounds and hidden behind them; a wave covers 256 / Q + 1 rows at most -- one or
// two on any real code -- so they are nearly wave-uniform, and 2 * 4096 floats stay in cache.
__global__ __launch_bounds__(kSimBlock) void sim_channel_awgn_mix(float *__restrict__ llr, long long batch, int n, unsigned Q,
                                                                  uint32_t k0, uint32_t k1, uint32_t stream_id,
                                                                  unsigned long long first_frame, unsigned p0, unsigned K,
                                                                  unsigned Kinv,
                                                                  const float *__restrict__ scale_tab,
                                                                  const float *__restrict__ shift_tab,
                                                                  const uint8_t *__restrict__ cw)
{
    const unsigned long long g0 = (unsigned long long)blockIdx.x * kSimBlock;     // first quad of the workgroup: uniform
    const unsigned long long b0 = g0 / Q;
    const unsigned t = (unsigned)(g0 - b0 * Q) + threadIdx.x;                     // < Q + 256 <= 2^29 + 256
    const unsigned db = t / Q;
    const long long b = (long long)b0 + db;
    const unsigned q = t - db * Q;
    if (b >= batch) return;
    const unsigned r = (unsigned)b + p0;
    unsigned p = r - __umulhi(r, Kinv) * K;                                       // in [0, 2K), see above
    if (p >= K) p -= K;                                                           // (first_frame + b) mod K
    const float scale = scale_tab[p], shift = shift_tab[p];
    const unsigned long long f = first_frame + (unsigned long long)b;
    uint32_t x[4];
    philox4x32_10((uint32_t)f, (uint32_t)(f >> 32), q, stream_id, k0, k1, x);
    float z[4];
    sim_box_muller(x[0], x[1], z[0], z[1]);
    sim_box_muller(x[2], x[3], z[2], z[3]);
    const int j0 = (int)(q * 4u);
    const int cnt = n - j0 < 4 ? n - j0 : 4;
    unsigned cbits = 0;                                                           // codeword bits j0 .. j0+3
    if (cw) cbits = (cw[j0 >> 3] >> (j0 & 7)) & 0xfu;                             // j0 % 8 is 0 or 4: one byte holds all four
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float y = fmaf(z[k], scale, shift);
        v[k] = ((cbits >> k) & 1u) ? -y : y;
    }
    sim_store_quad(llr + (size_t)b * (size_t)n + (size_t)j0, v, cnt);
}

// ------------------------------------------------------------------------------------------ rate matching
// ldpc_channel_awgn_rm / _mix_rm: the stream above with a punctured mask (the bit was not sent: LLR +0.0f, an erasure to the
// min-sum kernels) and a shortened mask (the bit is known: s_j * short_llr).  The Philox counter stays on the VARIABLE index
// j -- quad q of frame f draws the words it draws in sim_channel_awgn -- so every transmitted position holds the plain draw
// bit for bit and the profiles of a rate-compatible family see common noise.  The same lane-per-quad shape and stores as the
// plain kernels, which are left as they are.  A quad's four mask bits sit in one byte, as its codeword bits do (j0 % 8 is 0
// or 4); the three byte loads are issued before the Philox rounds.  A quad none of whose bits below n is transmitted skips
// the rounds and both Box-Muller pairs: a lane-level branch, so a contiguous punctured block of 64 quads or more frees whole
// waves and a scattered profile frees next to nothing.

// mask nibbles of quad j0 / 4: (codeword, punctured and not shortened, shortened), each four bits
__device__ inline void sim_rm_nibbles(int j0, const uint8_t *__restrict__ cw, const uint8_t *__restrict__ punct,
                                      const uint8_t *__restrict__ shrt, unsigned &cbits, unsigned &pbits, unsigned &sbits)
{
    const int byte = j0 >> 3, sh = j0 & 7;
    cbits = cw ? (cw[byte] >> sh) & 0xfu : 0u;
    sbits = shrt ? (shrt[byte] >> sh) & 0xfu : 0u;
    pbits = punct ? (punct[byte] >> sh) & 0xfu & ~sbits : 0u;                     // a bit in both masks is shortened
}

// the quad's four LLRs: the plain draw where the bit is transmitted.  `live` has bit k set for j0 + k < n, so the pad bits of a
// mask's last byte never keep a tail quad from being skipped (and are never stored)
__device__ inline void sim_rm_quad(unsigned long long f, unsigned q, uint32_t k0, uint32_t k1, uint32_t stream_id, float scale,
                                   float shift, float short_llr, unsigned cbits, unsigned pbits, unsigned sbits, unsigned live,
                                   float v[4])
{
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (((pbits | sbits) & live) != live) {                                       // a transmitted bit in the quad
        uint32_t x[4];
        philox4x32_10((uint32_t)f, (uint32_t)(f >> 32), q, stream_id, k0, k1, x);
        sim_box_muller(x[0], x[1], z[0], z[1]);
        sim_box_muller(x[2], x[3], z[2], z[3]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float y = fmaf(z[k], scale, shift);
        if ((sbits >> k) & 1u) y = short_llr;
        y = ((cbits >> k) & 1u) ? -y : y;
        v[k] = ((pbits >> k) & 1u) ? 0.0f : y;                                    // +0.0f whatever the codeword bit is
    }
}

__global__ __launch_bounds__(kSimBlock) void sim_channel_awgn_rm(float *__restrict__ llr, long long batch, int n, unsigned Q,
                                                                 uint32_t k0, uint32_t k1, uint32_t stream_id,
                                                                 unsigned long long first_frame, float scale, float shift,
                                                                 const uint8_t *__restrict__ cw,
                                                                 const uint8_t *__restrict__ punct,
                                                                 const uint8_t *__restrict__ shrt, float short_llr)
{
    const unsigned long long g0 = (unsigned long long)blockIdx.x * kSimBlock;     // first quad of the workgroup: uniform
    const unsigned long long b0 = g0 / Q;
    const unsigned t = (unsigned)(g0 - b0 * Q) + threadIdx.x;                     // < Q + 256 <= 2^29 + 256
    const unsigned db = t / Q;
    const long long b = (long long)b0 + db;
    const unsigned q = t - db * Q;
    if (b >= batch) return;
    const int j0 = (int)(q * 4u);
    const int cnt = n - j0 < 4 ? n - j0 : 4;
    unsigned cbits, pbits, sbits;
    sim_rm_nibbles(j0, cw, punct, shrt, cbits, pbits, sbits);
    float v[4];
    sim_rm_quad(first_frame + (unsigned long long)b, q, k0, k1, stream_id, scale, shift, short_llr, cbits, pbits, sbits,
                (1u << cnt) - 1u, v);
    sim_store_quad(llr + (size_t)b * (size_t)n + (size_t)j0, v, cnt);
}

__global__ __launch_bounds__(kSimBlock) void sim_channel_awgn_mix_rm(float *__restrict__ llr, long long batch, int n, unsigned Q,
                                                                     uint32_t k0, uint32_t k1, uint32_t stream_id,
                                                                     unsigned long long first_frame, unsigned p0, unsigned K,
                                                                     unsigned Kinv,
                                                                     const float *__restrict__ scale_tab,
                                                                     const float *__restrict__ shift_tab,
                                                                     const uint8_t *__restrict__ cw,
                                                                     const uint8_t *__restrict__ punct,
                                                                     const uint8_t *__restrict__ shrt, float short_llr)
{
    const unsigned long long g0 = (unsigned long long)blockIdx.x * kSimBlock;     // first quad of the workgroup: uniform
    const unsigned long long b0 = g0 / Q;
    const unsigned t = (unsigned)(g0 - b0 * Q) + threadIdx.x;                     // < Q + 256 <= 2^29 + 256
    const unsigned db = t / Q;
    const long long b = (long long)b0 + db;
    const unsigned q = t - db * Q;
    if (b >= batch) return;
    const unsigned r = (unsigned)b + p0;
    unsigned p = r - __umulhi(r, Kinv) * K;                                       // in [0, 2K), as in sim_channel_awgn_mix
    if (p >= K) p -= K;                                                           // (first_frame + b) mod K
    const float scale = scale_tab[p], shift = shift_tab[p];
    const int j0 = (int)(q * 4u);
    const int cnt = n - j0 < 4 ? n - j0 : 4;
    unsigned cbits, pbits, sbits;
    sim_rm_nibbles(j0, cw, punct, shrt, cbits, pbits, sbits);
    float v[4];
    sim_rm_quad(first_frame + (unsigned long long)b, q, k0, k1, stream_id, scale, shift, short_llr, cbits, pbits, sbits,
                (1u << cnt) - 1u, v);
    sim_store_quad(llr + (size_t)b * (size_t)n + (size_t)j0, v, cnt);
}

// the raw words of quad i: frame first_frame + i / quads_per_frame, quad i % quads_per_frame (ldpc_debug_philox)
__global__ __launch_bounds__(kSimBlock) void sim_debug_philox(uint32_t *__restrict__ out, long long count, uint32_t k0,
                                                              uint32_t k1, uint32_t stream_id, unsigned long long first_frame,
                                                              unsigned qpf)
{
    const long long i = (long long)blockIdx.x * kSimBlock + threadIdx.x;
    if (i >= count) return;
    const unsigned long long f = first_frame + (unsigned long long)i / qpf;
    uint32_t x[4];
    philox4x32_10((uint32_t)f, (uint32_t)(f >> 32), (uint32_t)((unsigned long long)i % qpf), stream_id, k0, k1, x);
    for (int k = 0; k < 4; ++k) out[(size_t)i * 4 + k] = x[k];
}

// ------------------------------------------------------------------------------------------ error counters
// state = { frames, frame_errors, bit_errors, iterations, done, blocks_seen, 0, 0 } (int64).  Two launches per block, in
// stream order, rather than one launch whose last-ticket workgroup folds: the entry point has no scratch for a ticket and
// per-frame results (the state is all the caller gives), and the order of two launches needs no fence or ticket at all.
//   sim_count_frames (grid)  : per-frame popcounts over the frames the room allows (take0), summed WITHOUT order into
//                              state[3] (iterations) and the two spare words state[6] (frame errors) and state[7] (bit
//                              errors); it reads state[0], [1], [4], which no workgroup of it writes.
//   sim_count_fold (1 group) : applies the stop rule.  As long as the block's frame errors stay below what max_errors
//                              still allows -- every block of a point but its last -- the unordered sums ARE the ordered
//                              ones and are folded in O(1).  Otherwise it walks the block in order (1024 frames per step,
//                              popcounts recomputed wave per row, a ballot prefix over the frame-error flags), finds the
//                              frame that reaches the limit and takes the frames after it back out of the sums.

__device__ inline int sim_wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// bytes off .. off+3 of a row of rb bytes as one little-endian word (rows have no alignment; short at the row's end)
__device__ inline uint32_t sim_row_word(const uint8_t *__restrict__ row, int rb, int off)
{
    uint32_t w = 0;
    if (off + 4 <= rb) {
        __builtin_memcpy(&w, row + off, 4);
    } else {
        for (int k = 0; k < rb - off; ++k) w |= (uint32_t)row[off + k] << (8 * k);
    }
    return w;
}

// wrong bits of one frame, by the 64 lanes of a wave (every lane returns the sum); bits >= n are masked off
__device__ inline int sim_row_wrong(const uint8_t *__restrict__ row, const uint8_t *__restrict__ cw, int rb, int n, int lane)
{
    int cnt = 0;
    for (int off = lane * 4; off < rb; off += 256) {
        uint32_t w = sim_row_word(row, rb, off);
        if (cw) w ^= sim_row_word(cw, rb, off);
        const long long nb = (long long)n - 8ll * off;                 // >= 1: off < rb = ceil(n / 8)
        if (nb < 32) w &= (1u << nb) - 1u;
        cnt += __popc(w);
    }
    return sim_wave_sum(cnt);
}

// frames of this block the room allows, before the error limit is looked at; 0 once the point is done
__device__ inline long long sim_take0(const long long *state, long long B, long long max_frames, long long max_errors)
{
    if (state[4] != 0 || state[0] >= max_frames || state[1] >= max_errors) return 0;
    const long long room = max_frames - state[0];
    return B < room ? B : room;
}

__global__ __launch_bounds__(kSimBlock) void sim_count_frames(long long *state, const uint8_t *__restrict__ packed,
                                                              const int *__restrict__ iters, long long B, int n, int rb,
                                                              const uint8_t *__restrict__ cw, long long max_frames,
                                                              long long max_errors)
{
    const long long take0 = sim_take0(state, B, max_frames, max_errors);
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (kSimBlock / 64) + (threadIdx.x >> 6);
    const long long stride = (long long)gridDim.x * (kSimBlock / 64) * 64;
    long long s_ferr = 0, s_wrong = 0;          // wave-uniform
    int my_it = 0;                              // <= (rows of this lane) * T
    long long s_it = 0;
    for (long long base = wave * 64; base < take0; base += stride) {
        const int rows = take0 - base < 64 ? (int)(take0 - base) : 64;
        my_it = lane < rows ? iters[base + lane] : 0;
        s_it += sim_wave_sum(my_it);
        for (int k = 0; k < rows; ++k) {
            const int w = sim_row_wrong(packed + (size_t)(base + k) * (size_t)rb, cw, rb, n, lane);
            s_wrong += w;
            s_ferr += w > 0;
        }
    }
    if (lane == 0) {
        unsigned long long *st = reinterpret_cast<unsigned long long *>(state);
        if (s_it) atomicAdd(&st[3], (unsigned long long)s_it);
        if (s_ferr) atomicAdd(&st[6], (unsigned long long)s_ferr);
        if (s_wrong) atomicAdd(&st[7], (unsigned long long)s_wrong);
    }
}

__global__ __launch_bounds__(kSimFoldBlock) void sim_count_fold(long long *state, const uint8_t *__restrict__ packed,
                                                                const int *__restrict__ iters, long long B, int n, int rb,
                                                                const uint8_t *__restrict__ cw, long long max_frames,
                                                                long long max_errors)
{
    constexpr int kWaves = kSimFoldBlock / 64;
    __shared__ int sh_cnt[kWaves];
    __shared__ long long sh_sum[kWaves][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long frames0 = state[0], errors0 = state[1], done0 = state[4];
    const long long take0 = sim_take0(state, B, max_frames, max_errors);
    const long long e = state[6], w = state[7];
    long long take = take0, d_ferr = e, d_wrong = w, d_it = 0;
    if (take0 > 0 && errors0 + e >= max_errors) {        // the error limit falls inside this block: uniform branch
        const long long need = max_errors - errors0;     // >= 1 (take0 > 0)
        long long cum = 0;                               // frame errors before this step
        long long acc[4] = {0, 0, 0, 0};                 // per thread: frames kept; frame errors, wrong bits, iterations taken back
        for (long long tile = 0; tile < take0; tile += kSimFoldBlock) {
            const long long wbase = tile + (long long)wv * 64;
            const int rows = take0 - wbase < 64 ? (take0 - wbase > 0 ? (int)(take0 - wbase) : 0) : 64;
            int mine = 0;                                // wrong bits of frame tile + tid
            for (int k = 0; k < rows; ++k) {
                const int c = sim_row_wrong(packed + (size_t)(wbase + k) * (size_t)rb, cw, rb, n, lane);
                if (lane == k) mine = c;
            }
            const bool valid = lane < rows;
            const int ferr = valid && mine > 0;
            const unsigned long long bal = __ballot(ferr);
            const int incl = __popcll(bal & ((2ull << lane) - 1ull));
            if (lane == 0) sh_cnt[wv] = __popcll(bal);
            __syncthreads();
            int before = 0, total = 0;
            for (int k = 0; k < kWaves; ++k) {
                before += k < wv ? sh_cnt[k] : 0;
                total += sh_cnt[k];
            }
            __syncthreads();
            if (valid) {
                if (cum + before + incl - ferr < need) {  // fewer than `need` frame errors before this frame: it is consumed
                    acc[0] += 1;
                } else {
                    acc[1] += ferr;
                    acc[2] += mine;
                    acc[3] += iters[wbase + lane];
                }
            }
            cum += total;
        }
        for (int k = 0; k < 4; ++k) {
            long long v = acc[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) sh_sum[wv][k] = v;
        }
        __syncthreads();
        long long tot[4] = {0, 0, 0, 0};
        for (int k = 0; k < kWaves; ++k)
            for (int c = 0; c < 4; ++c) tot[c] += sh_sum[k][c];
        take = tot[0];
        d_ferr = e - tot[1];
        d_wrong = w - tot[2];
        d_it = -tot[3];
    }
    __syncthreads();                                     // every thread has read the state
    if (tid == 0) {
        const long long frames = frames0 + take, fe = errors0 + d_ferr;
        state[0] = frames;
        state[1] = fe;
        state[2] += d_wrong;
        state[3] += d_it;
        state[4] = (done0 != 0 || frames >= max_frames || fe >= max_errors) ? 1 : 0;
        state[5] += 1;
        state[6] = 0;
        state[7] = 0;
    }
}

// ------------------------------------------------------------------------------------------ diagnostic counters
// ldpc_sim_count_diag: the same two launches, the same state, plus diag = { undetected, captured, 0, 0, hist[T + 1],
// records[capture][4] } (include/ldpc_hip.h).  What is added to each launch:
//   sim_diag_frames (grid)  : one word per frame into scratch -- wrong bits in bits 0..30, the success flag in bit 31 (n and T
//                             are both full int32 ranges, so the iteration count stays where it is, in iterations[]) -- so the
//                             fold never reads a packed row; the iterations binned in an LDS histogram of T + 1 counters per
//                             workgroup (dynamic shared memory; above kSimDiagLdsBins bins straight into the global one), each
//                             non-empty bin flushed with one global atomic; undetected errors summed WITHOUT order into diag[2].
//   sim_diag_fold (1 group) : O(1) when no stop frame falls inside the block and there is nothing to record (no frame error in
//                             it, or the capture full).  Otherwise it walks the per-frame words, 1024 frames per step; the
//                             ballot prefix of the stop rule is the ordinal of each frame error: a consumed one whose ordinal is
//                             below `capture` writes its record, a frame past the stop frame is taken back out of the sums, the
//                             undetected count and the histogram.

constexpr int kSimDiagLdsBins = 8192;   // 32 KiB of LDS at most: two workgroups of the grid pass per CU stay possible

__device__ inline int sim_clamp_bin(int it, int T) { return it < 0 ? 0 : (it > T ? T : it); }

__global__ __launch_bounds__(kSimBlock) void sim_diag_frames(long long *state, long long *diag, int T, int lds_bins,
                                                             uint32_t *__restrict__ words, const uint8_t *__restrict__ packed,
                                                             const int *__restrict__ iters, const uint8_t *__restrict__ success,
                                                             long long B, int n, int rb, const uint8_t *__restrict__ cw,
                                                             long long max_frames, long long max_errors)
{
    extern __shared__ unsigned sim_hist[];      // lds_bins counters (T + 1, or none)
    unsigned long long *hist = reinterpret_cast<unsigned long long *>(diag) + 4;
    for (int t = threadIdx.x; t < lds_bins; t += kSimBlock) sim_hist[t] = 0;
    __syncthreads();
    const long long take0 = sim_take0(state, B, max_frames, max_errors);
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (kSimBlock / 64) + (threadIdx.x >> 6);
    const long long stride = (long long)gridDim.x * (kSimBlock / 64) * 64;
    long long s_ferr = 0, s_wrong = 0, s_und = 0, s_it = 0;      // wave-uniform
    for (long long base = wave * 64; base < take0; base += stride) {
        const int rows = take0 - base < 64 ? (int)(take0 - base) : 64;
        int mine = 0;                           // wrong bits of frame base + lane
        for (int k = 0; k < rows; ++k) {
            const int w = sim_row_wrong(packed + (size_t)(base + k) * (size_t)rb, cw, rb, n, lane);
            s_wrong += w;
            s_ferr += w > 0;
            if (lane == k) mine = w;
        }
        int my_it = 0, und = 0;
        if (lane < rows) {
            my_it = iters[base + lane];
            const unsigned ok = success[base + lane] != 0;
            und = mine > 0 && ok;
            words[base + lane] = (uint32_t)mine | (ok << 31);
            const int bin = sim_clamp_bin(my_it, T);
            if (lds_bins) atomicAdd(&sim_hist[bin], 1u);
            else atomicAdd(&hist[bin], 1ull);
        }
        s_it += sim_wave_sum(my_it);
        s_und += __popcll(__ballot(und));
    }
    if (lane == 0) {
        unsigned long long *st = reinterpret_cast<unsigned long long *>(state);
        if (s_it) atomicAdd(&st[3], (unsigned long long)s_it);
        if (s_ferr) atomicAdd(&st[6], (unsigned long long)s_ferr);
        if (s_wrong) atomicAdd(&st[7], (unsigned long long)s_wrong);
        if (s_und) atomicAdd(reinterpret_cast<unsigned long long *>(diag) + 2, (unsigned long long)s_und);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < lds_bins; t += kSimBlock) {
        const unsigned c = sim_hist[t];
        if (c) atomicAdd(&hist[t], (unsigned long long)c);
    }
}

__global__ __launch_bounds__(kSimFoldBlock) void sim_diag_fold(long long *state, long long *diag, int T, long long capture,
                                                               const uint32_t *__restrict__ words,
                                                               const int *__restrict__ iters, long long B,
                                                               unsigned long long first_frame, long long max_frames,
                                                               long long max_errors)
{
    constexpr int kWaves = kSimFoldBlock / 64;
    __shared__ int sh_cnt[kWaves];
    __shared__ long long sh_sum[kWaves][5];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long frames0 = state[0], errors0 = state[1], done0 = state[4];
    const long long take0 = sim_take0(state, B, max_frames, max_errors);
    const long long e = state[6], w = state[7], u = diag[2], captured0 = diag[1];
    long long take = take0, d_ferr = e, d_wrong = w, d_it = 0, d_und = u;
    const bool stop = take0 > 0 && errors0 + e >= max_errors;           // the error limit falls inside this block
    if (stop || (take0 > 0 && e > 0 && captured0 < capture)) {           // uniform branch
        const long long need = max_errors - errors0;                     // >= 1 (take0 > 0)
        long long *rec = diag + 4 + (long long)T + 1;
        unsigned long long *hist = reinterpret_cast<unsigned long long *>(diag) + 4;
        long long cum = 0;                                               // frame errors before this step
        long long acc[5] = {0, 0, 0, 0, 0};   // per thread: frames kept; frame errors, wrong bits, iterations, undetected taken back
        for (long long tile = 0; tile < take0; tile += kSimFoldBlock) {
            if (!stop && captured0 + cum >= capture) break;              // capture full and nothing to take back: uniform
            const long long row = tile + tid;
            const bool valid = row < take0;
            const uint32_t word = valid ? words[row] : 0u;
            const int mine = (int)(word & 0x7fffffffu);
            const int ferr = mine > 0;
            const unsigned long long bal = __ballot(ferr);
            const int incl = __popcll(bal & ((2ull << lane) - 1ull));
            if (lane == 0) sh_cnt[wv] = __popcll(bal);
            __syncthreads();
            int before = 0, total = 0;
            for (int k = 0; k < kWaves; ++k) {
                before += k < wv ? sh_cnt[k] : 0;
                total += sh_cnt[k];
            }
            __syncthreads();
            if (valid) {
                const long long ordinal = cum + before + incl - ferr;   // frame errors of this block before this frame
                const int und = ferr && (word >> 31);
                if (!stop || ordinal < need) {                           // consumed
                    acc[0] += 1;
                    const long long k = captured0 + ordinal;
                    if (ferr && k < capture) {
                        long long *r = rec + 4 * k;
                        r[0] = (long long)(first_frame + (unsigned long long)row);
                        r[1] = mine;
                        r[2] = iters[row];
                        r[3] = und;
                    }
                } else {
                    const int it = iters[row];
                    acc[1] += ferr;
                    acc[2] += mine;
                    acc[3] += it;
                    acc[4] += und;
                    atomicAdd(&hist[sim_clamp_bin(it, T)], ~0ull);       // minus one: the grid pass counted this frame
                }
            }
            cum += total;
        }
        if (stop) {
            for (int k = 0; k < 5; ++k) {
                long long v = acc[k];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == 0) sh_sum[wv][k] = v;
            }
            __syncthreads();
            long long tot[5] = {0, 0, 0, 0, 0};
            for (int k = 0; k < kWaves; ++k)
                for (int c = 0; c < 5; ++c) tot[c] += sh_sum[k][c];
            take = tot[0];
            d_ferr = e - tot[1];
            d_wrong = w - tot[2];
            d_it = -tot[3];
            d_und = u - tot[4];
        }
    }
    __syncthreads();                                     // every thread has read the state and the diag header
    if (tid == 0) {
        const long long frames = frames0 + take, fe = errors0 + d_ferr;
        state[0] = frames;
        state[1] = fe;
        state[2] += d_wrong;
        state[3] += d_it;
        state[4] = (done0 != 0 || frames >= max_frames || fe >= max_errors) ? 1 : 0;
        state[5] += 1;
        state[6] = 0;
        state[7] = 0;
        if (take0 > 0) {                                 // a launch that finds the point done leaves diag alone
            const long long captured = captured0 + d_ferr;
            diag[0] += d_und;
            diag[1] = captured < capture ? captured : capture;
            diag[2] = 0;
        }
    }
}

// ------------------------------------------------------------------------------------------ masked counters
// ldpc_sim_count_rm / _diag_rm with a count mask: wrong = popcount((packed XOR codeword) AND mask) over bits < n, and that
// number in the place of `wrong` everywhere -- frame errors, the stop rule, undetected errors, the records.  The kernels that
// read packed rows are restated with the mask; sim_diag_fold reads the per-frame words only and serves both.  Without a mask
// the entry points launch the plain kernels above, which are left as they are.

__device__ inline int sim_row_wrong_rm(const uint8_t *__restrict__ row, const uint8_t *__restrict__ cw,
                                       const uint8_t *__restrict__ mask, int rb, int n, int lane)
{
    int cnt = 0;
    for (int off = lane * 4; off < rb; off += 256) {
        uint32_t w = sim_row_word(row, rb, off);
        if (cw) w ^= sim_row_word(cw, rb, off);
        w &= sim_row_word(mask, rb, off);
        const long long nb = (long long)n - 8ll * off;                 // >= 1: off < rb = ceil(n / 8)
        if (nb < 32) w &= (1u << nb) - 1u;
        cnt += __popc(w);
    }
    return sim_wave_sum(cnt);
}

__global__ __launch_bounds__(kSimBlock) void sim_count_frames_rm(long long *state, const uint8_t *__restrict__ packed,
                                                                 const int *__restrict__ iters, long long B, int n, int rb,
                                                                 const uint8_t *__restrict__ cw,
                                                                 const uint8_t *__restrict__ mask, long long max_frames,
                                                                 long long max_errors)
{
    const long long take0 = sim_take0(state, B, max_frames, max_errors);
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (kSimBlock / 64) + (threadIdx.x >> 6);
    const long long stride = (long long)gridDim.x * (kSimBlock / 64) * 64;
    long long s_ferr = 0, s_wrong = 0, s_it = 0;                       // wave-uniform
    for (long long base = wave * 64; base < take0; base += stride) {
        const int rows = take0 - base < 64 ? (int)(take0 - base) : 64;
        s_it += sim_wave_sum(lane < rows ? iters[base + lane] : 0);
        for (int k = 0; k < rows; ++k) {
            const int w = sim_row_wrong_rm(packed + (size_t)(base + k) * (size_t)rb, cw, mask, rb, n, lane);
            s_wrong += w;
            s_ferr += w > 0;
        }
    }
    if (lane == 0) {
        unsigned long long *st = reinterpret_cast<unsigned long long *>(state);
        if (s_it) atomicAdd(&st[3], (unsigned long long)s_it);
        if (s_ferr) atomicAdd(&st[6], (unsigned long long)s_ferr);
        if (s_wrong) atomicAdd(&st[7], (unsigned long long)s_wrong);
    }
}

__global__ __launch_bounds__(kSimFoldBlock) void sim_count_fold_rm(long long *state, const uint8_t *__restrict__ packed,
                                                                   const int *__restrict__ iters, long long B, int n, int rb,
                                                                   const uint8_t *__restrict__ cw,
                                                                   const uint8_t *__restrict__ mask, long long max_frames,
                                                                   long long max_errors)
{
    constexpr int kWaves = kSimFoldBlock / 64;
    __shared__ int sh_cnt[kWaves];
    __shared__ long long sh_sum[kWaves][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long frames0 = state[0], errors0 = state[1], done0 = state[4];
    const long long take0 = sim_take0(state, B, max_frames, max_errors);
    const long long e = state[6], w = state[7];
    long long take = take0, d_ferr = e, d_wrong = w, d_it = 0;
    if (take0 > 0 && errors0 + e >= max_errors) {        // the error limit falls inside this block: uniform branch
        const long long need = max_errors - errors0;     // >= 1 (take0 > 0)
        long long cum = 0;                               // frame errors before this step
        long long acc[4] = {0, 0, 0, 0};                 // per thread: frames kept; frame errors, wrong bits, iterations taken back
        for (long long tile = 0; tile < take0; tile += kSimFoldBlock) {
            const long long wbase = tile + (long long)wv * 64;
            const int rows = take0 - wbase < 64 ? (take0 - wbase > 0 ? (int)(take0 - wbase) : 0) : 64;
            int mine = 0;                                // masked wrong bits of frame tile + tid
            for (int k = 0; k < rows; ++k) {
                const int c = sim_row_wrong_rm(packed + (size_t)(wbase + k) * (size_t)rb, cw, mask, rb, n, lane);
                if (lane == k) mine = c;
            }
            const bool valid = lane < rows;
            const int ferr = valid && mine > 0;
            const unsigned long long bal = __ballot(ferr);
            const int incl = __popcll(bal & ((2ull << lane) - 1ull));
            if (lane == 0) sh_cnt[wv] = __popcll(bal);
            __syncthreads();
            int before = 0, total = 0;
            for (int k = 0; k < kWaves; ++k) {
                before += k < wv ? sh_cnt[k] : 0;
                total += sh_cnt[k];
            }
            __syncthreads();
            if (valid) {
                if (cum + before + incl - ferr < need) {  // fewer than `need` frame errors before this frame: it is consumed
                    acc[0] += 1;
                } else {
                    acc[1] += ferr;
                    acc[2] += mine;
                    acc[3] += iters[wbase + lane];
                }
            }
            cum += total;
        }
        for (int k = 0; k < 4; ++k) {
            long long v = acc[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) sh_sum[wv][k] = v;
        }
        __syncthreads();
        long long tot[4] = {0, 0, 0, 0};
        for (int k = 0; k < kWaves; ++k)
            for (int c = 0; c < 4; ++c) tot[c] += sh_sum[k][c];
        take = tot[0];
        d_ferr = e - tot[1];
        d_wrong = w - tot[2];
        d_it = -tot[3];
    }
    __syncthreads();                                     // every thread has read the state
    if (tid == 0) {
        const long long frames = frames0 + take, fe = errors0 + d_ferr;
        state[0] = frames;
        state[1] = fe;
        state[2] += d_wrong;
        state[3] += d_it;
        state[4] = (done0 != 0 || frames >= max_frames || fe >= max_errors) ? 1 : 0;
        state[5] += 1;
        state[6] = 0;
        state[7] = 0;
    }
}

__global__ __launch_bounds__(kSimBlock) void sim_diag_frames_rm(long long *state, long long *diag, int T, int lds_bins,
                                                                uint32_t *__restrict__ words,
                                                                const uint8_t *__restrict__ packed,
                                                                const int *__restrict__ iters,
                                                                const uint8_t *__restrict__ success, long long B, int n, int rb,
                                                                const uint8_t *__restrict__ cw,
                                                                const uint8_t *__restrict__ mask, long long max_frames,
                                                                long long max_errors)
{
    extern __shared__ unsigned sim_hist[];      // lds_bins counters (T + 1, or none)
    unsigned long long *hist = reinterpret_cast<unsigned long long *>(diag) + 4;
    for (int t = threadIdx.x; t < lds_bins; t += kSimBlock) sim_hist[t] = 0;
    __syncthreads();
    const long long take0 = sim_take0(state, B, max_frames, max_errors);
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (kSimBlock / 64) + (threadIdx.x >> 6);
    const long long stride = (long long)gridDim.x * (kSimBlock / 64) * 64;
    long long s_ferr = 0, s_wrong = 0, s_und = 0, s_it = 0;      // wave-uniform
    for (long long base = wave * 64; base < take0; base += stride) {
        const int rows = take0 - base < 64 ? (int)(take0 - base) : 64;
        int mine = 0;                           // masked wrong bits of frame base + lane
        for (int k = 0; k < rows; ++k) {
            const int w = sim_row_wrong_rm(packed + (size_t)(base + k) * (size_t)rb, cw, mask, rb, n, lane);
            s_wrong += w;
            s_ferr += w > 0;
            if (lane == k) mine = w;
        }
        int my_it = 0, und = 0;
        if (lane < rows) {
            my_it = iters[base + lane];
            const unsigned ok = success[base + lane] != 0;
            und = mine > 0 && ok;
            words[base + lane] = (uint32_t)mine | (ok << 31);
            const int bin = sim_clamp_bin(my_it, T);
            if (lds_bins) atomicAdd(&sim_hist[bin], 1u);
            else atomicAdd(&hist[bin], 1ull);
        }
        s_it += sim_wave_sum(my_it);
        s_und += __popcll(__ballot(und));
    }
    if (lane == 0) {
        unsigned long long *st = reinterpret_cast<unsigned long long *>(state);
        if (s_it) atomicAdd(&st[3], (unsigned long long)s_it);
        if (s_ferr) atomicAdd(&st[6], (unsigned long long)s_ferr);
        if (s_wrong) atomicAdd(&st[7], (unsigned long long)s_wrong);
        if (s_und) atomicAdd(reinterpret_cast<unsigned long long *>(diag) + 2, (unsigned long long)s_und);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < lds_bins; t += kSimBlock) {
        const unsigned c = sim_hist[t];
        if (c) atomicAdd(&hist[t], (unsigned long long)c);
    }
}

}  // namespace ldpc

namespace {

int sim_channel_launch(float *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                       float scale, float shift, const uint8_t *cw, hipStream_t s)
{
    const unsigned Q = ((unsigned)n + 3u) / 4u;
    const unsigned long long quads = (unsigned long long)batch * Q;
    const unsigned long long blocks = (quads + kSimBlock - 1) / kSimBlock;
    if (blocks > 0x7fffffffull) return fail(LDPC_ERR_UNSUPPORTED, "batch too large for one launch");
    hipLaunchKernelGGL(sim_channel_awgn, dim3((unsigned)blocks), dim3(kSimBlock), 0, s, llr, (long long)batch, (int)n, Q,
                       (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, (unsigned long long)first_frame, scale, shift, cw);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int sim_channel_mix_launch(float *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                           const float *scale_tab, const float *shift_tab, int32_t n_points, const uint8_t *cw, hipStream_t s)
{
    const unsigned Q = ((unsigned)n + 3u) / 4u;
    const unsigned long long quads = (unsigned long long)batch * Q;
    const unsigned long long blocks = (quads + kSimBlock - 1) / kSimBlock;
    if (blocks > 0x7fffffffull) return fail(LDPC_ERR_UNSUPPORTED, "batch too large for one launch");
    const unsigned K = (unsigned)n_points;
    hipLaunchKernelGGL(sim_channel_awgn_mix, dim3((unsigned)blocks), dim3(kSimBlock), 0, s, llr, (long long)batch, (int)n, Q,
                       (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, (unsigned long long)first_frame,
                       (unsigned)(first_frame % K), K, 0xffffffffu / K, scale_tab, shift_tab, cw);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

// a rate-matching profile is usable: short_llr finite and > 0 wherever something is shortened (NULL: no rate matching)
int sim_rm_check(const ldpc_rate_match *rm)
{
    if (rm && rm->shortened_packed && !(std::isfinite(rm->short_llr) && rm->short_llr > 0.0f))
        return fail(LDPC_ERR_ARG, "short_llr must be finite and > 0 when shortened_packed is given");
    return LDPC_OK;
}

int sim_channel_rm_launch(float *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                          float scale, float shift, const uint8_t *cw, const ldpc_rate_match *rm, hipStream_t s)
{
    if (!rm) return sim_channel_launch(llr, batch, n, seed, stream_id, first_frame, scale, shift, cw, s);
    const unsigned Q = ((unsigned)n + 3u) / 4u;
    const unsigned long long quads = (unsigned long long)batch * Q;
    const unsigned long long blocks = (quads + kSimBlock - 1) / kSimBlock;
    if (blocks > 0x7fffffffull) return fail(LDPC_ERR_UNSUPPORTED, "batch too large for one launch");
    hipLaunchKernelGGL(sim_channel_awgn_rm, dim3((unsigned)blocks), dim3(kSimBlock), 0, s, llr, (long long)batch, (int)n, Q,
                       (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, (unsigned long long)first_frame, scale, shift, cw,
                       rm->punctured_packed, rm->shortened_packed, rm->shortened_packed ? rm->short_llr : 0.0f);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int sim_channel_mix_rm_launch(float *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                              const float *scale_tab, const float *shift_tab, int32_t n_points, const uint8_t *cw,
                              const ldpc_rate_match *rm, hipStream_t s)
{
    if (!rm) return sim_channel_mix_launch(llr, batch, n, seed, stream_id, first_frame, scale_tab, shift_tab, n_points, cw, s);
    const unsigned Q = ((unsigned)n + 3u) / 4u;
    const unsigned long long quads = (unsigned long long)batch * Q;
    const unsigned long long blocks = (quads + kSimBlock - 1) / kSimBlock;
    if (blocks > 0x7fffffffull) return fail(LDPC_ERR_UNSUPPORTED, "batch too large for one launch");
    const unsigned K = (unsigned)n_points;
    hipLaunchKernelGGL(sim_channel_awgn_mix_rm, dim3((unsigned)blocks), dim3(kSimBlock), 0, s, llr, (long long)batch, (int)n, Q,
                       (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, (unsigned long long)first_frame,
                       (unsigned)(first_frame % K), K, 0xffffffffu / K, scale_tab, shift_tab, cw, rm->punctured_packed,
                       rm->shortened_packed, rm->shortened_packed ? rm->short_llr : 0.0f);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

// mask: the count mask of a rate-matching profile, or NULL for the plain kernels
int sim_count_launch(int64_t *state, const uint8_t *packed, const int32_t *iters, int64_t batch, int32_t n,
                     const uint8_t *cw, int64_t max_frames, int64_t max_errors, hipStream_t s, const uint8_t *mask = nullptr)
{
    const int rb = (int)(((int64_t)n + 7) / 8);
    const long long groups = (batch + kSimBlock - 1) / kSimBlock;            // 64 frames per wave and pass
    const dim3 grid((unsigned)std::min<long long>(groups, 2048));
    if (batch > 0 && mask) {
        hipLaunchKernelGGL(sim_count_frames_rm, grid, dim3(kSimBlock), 0, s, (long long *)state, packed, iters,
                           (long long)batch, (int)n, rb, cw, mask, (long long)max_frames, (long long)max_errors);
        HIP_TRY(hipGetLastError());
    } else if (batch > 0) {
        hipLaunchKernelGGL(sim_count_frames, grid, dim3(kSimBlock), 0, s, (long long *)state, packed, iters,
                           (long long)batch, (int)n, rb, cw, (long long)max_frames, (long long)max_errors);
        HIP_TRY(hipGetLastError());
    }
    if (batch > 0 && mask)
        hipLaunchKernelGGL(sim_count_fold_rm, dim3(1), dim3(kSimFoldBlock), 0, s, (long long *)state, packed, iters,
                           (long long)batch, (int)n, rb, cw, mask, (long long)max_frames, (long long)max_errors);
    else                                                 // an empty block reads no row: the plain fold latches `done`
        hipLaunchKernelGGL(sim_count_fold, dim3(1), dim3(kSimFoldBlock), 0, s, (long long *)state, packed, iters,
                           (long long)batch, (int)n, rb, cw, (long long)max_frames, (long long)max_errors);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

size_t sim_diag_words(int32_t T, int64_t capture)
{
    if (T < 0 || capture < 0 || capture > (INT64_MAX >> 6)) return 0;
    return (size_t)4 + (size_t)T + 1 + 4 * (size_t)capture;
}

size_t sim_diag_scratch_bytes(int64_t batch) { return batch > 0 ? align_up((size_t)batch * sizeof(uint32_t)) : 0; }

int sim_count_diag_launch(int64_t *state, int64_t *diag, int32_t T, int64_t capture, const uint8_t *packed, const int32_t *iters,
                          const uint8_t *success, int64_t batch, int32_t n, const uint8_t *cw, uint64_t first_frame,
                          int64_t max_frames, int64_t max_errors, uint32_t *words, hipStream_t s,
                          const uint8_t *mask = nullptr)
{
    if (batch == 0)                                      // nothing to bin or record: the plain fold moves the state alone
        return sim_count_launch(state, packed, iters, 0, n, cw, max_frames, max_errors, s);
    const int rb = (int)(((int64_t)n + 7) / 8);
    const int lds_bins = (int64_t)T + 1 <= kSimDiagLdsBins ? T + 1 : 0;
    const long long groups = (batch + kSimBlock - 1) / kSimBlock;            // 64 frames per wave and pass
    const dim3 grid((unsigned)std::min<long long>(groups, 2048));
    if (mask)
        hipLaunchKernelGGL(sim_diag_frames_rm, grid, dim3(kSimBlock), (size_t)lds_bins * sizeof(unsigned), s, (long long *)state,
                           (long long *)diag, (int)T, lds_bins, words, packed, iters, success, (long long)batch, (int)n, rb, cw,
                           mask, (long long)max_frames, (long long)max_errors);
    else
        hipLaunchKernelGGL(sim_diag_frames, grid, dim3(kSimBlock), (size_t)lds_bins * sizeof(unsigned), s, (long long *)state,
                           (long long *)diag, (int)T, lds_bins, words, packed, iters, success, (long long)batch, (int)n, rb, cw,
                           (long long)max_frames, (long long)max_errors);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sim_diag_fold, dim3(1), dim3(kSimFoldBlock), 0, s, (long long *)state, (long long *)diag, (int)T,
                       (long long)capture, (const uint32_t *)words, iters, (long long)batch, (unsigned long long)first_frame,
                       (long long)max_frames, (long long)max_errors);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

// workspace of ldpc_simulate for blocks of `block` frames: LLR rows, packed decisions, iterations, the state, the decoder's own
// ldpc_simulate_diag (capture >= 0) adds a success row, the per-frame words and the diag buffer behind them
struct SimWorkspace {
    size_t o_llr = 0, o_packed = 0, o_iters = 0, o_state = 0, o_dec = 0, dec_bytes = 0, total = 0;
    size_t o_success = 0, o_words = 0, o_diag = 0, diag_words = 0;
};

SimWorkspace sim_carve(const ldpc_decoder *d, int64_t block, int64_t capture = -1)
{
    SimWorkspace w;
    const size_t n = (size_t)d->g->n, b = (size_t)block;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off += align_up(bytes);
        return o;
    };
    w.o_llr = take(b * n * sizeof(float));
    w.o_packed = take(b * ((n + 7) / 8));
    w.o_iters = take(b * sizeof(int32_t));
    w.o_state = take(8 * sizeof(int64_t));
    w.dec_bytes = ldpc_decoder_workspace_bytes(d, block);
    w.o_dec = take(w.dec_bytes);
    if (capture >= 0) {
        w.o_success = take(b);
        w.o_words = take(sim_diag_scratch_bytes(block));
        w.diag_words = sim_diag_words(d->T, capture);
        w.o_diag = take(w.diag_words * sizeof(int64_t));
    }
    w.total = off;
    return w;
}

struct PinnedState {
    int64_t *p = nullptr;
    ~PinnedState()
    {
        if (p) (void)hipHostFree(p);
    }
};

// the host loop of ldpc_simulate (capture < 0, out_diag unused) and of ldpc_simulate_diag (capture >= 0); rm: the profile of
// the _rm forms, NULL for the plain ones -- which then launch exactly what they launched before the profile existed
int simulate_impl(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_rate_match *rm, int64_t capture,
                  int64_t out_state[8], int64_t *out_diag, void *workspace, size_t workspace_bytes, void *stream)
{
    const bool diagnostics = capture >= 0;
    if (!d || !desc || !out_state) return fail(LDPC_ERR_ARG, "NULL decoder / descriptor / out_state");
    if (diagnostics && !out_diag) return fail(LDPC_ERR_ARG, "NULL out_diag");
    if (diagnostics && sim_diag_words(d->T, capture) == 0) return fail(LDPC_ERR_ARG, "capture too large");
    if (int rc = sim_rm_check(rm)) return rc;
    const uint8_t *mask = rm ? rm->count_packed : nullptr;
    if (desc->block < 1) return fail(LDPC_ERR_ARG, "block < 1");
    if (desc->poll_blocks < 1) return fail(LDPC_ERR_ARG, "poll_blocks < 1");
    if (d->dtype != LDPC_F32) return fail(LDPC_ERR_UNSUPPORTED, "ldpc_simulate draws fp32 LLRs: float64 decoders are not supported");
    if (d->g->n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (!workspace) return fail(LDPC_ERR_ARG, "NULL workspace");
    if (((uintptr_t)workspace % kAlign) != 0) return fail(LDPC_ERR_ARG, "workspace must be %zu-byte aligned", kAlign);
    const SimWorkspace w = sim_carve(d, desc->block, capture);
    if (w.total > workspace_bytes) return fail(LDPC_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, w.total);
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
    const int32_t n = d->g->n;
    PinnedState host;
    HIP_TRY(hipHostMalloc((void **)&host.p, 8 * sizeof(int64_t), hipHostMallocDefault));
    HIP_TRY(hipMemsetAsync(state, 0, 8 * sizeof(int64_t), s));
    if (diagnostics) HIP_TRY(hipMemsetAsync(diag, 0, w.diag_words * sizeof(int64_t), s));
    auto count = [&](int64_t frames, int64_t first) {    // fold one decoded block (frames = 0: latch `done`)
        if (diagnostics)
            return sim_count_diag_launch(state, diag, d->T, capture, packed, iters, success, frames, n, desc->codeword_packed,
                                         desc->first_frame + (uint64_t)first, desc->max_frames, desc->max_errors, words, s,
                                         mask);
        return sim_count_launch(state, packed, iters, frames, n, desc->codeword_packed, desc->max_frames, desc->max_errors, s,
                                mask);
    };
    int64_t drawn = 0;                                   // frames drawn so far: block k starts at first_frame + k * block
    for (;;) {
        int queued = 0;
        for (int p = 0; p < desc->poll_blocks && drawn < desc->max_frames; ++p, ++queued) {
            const int64_t frames = std::min<int64_t>(desc->block, desc->max_frames - drawn);
            if (int rc = sim_channel_rm_launch(llr, frames, n, desc->seed, desc->stream_id, desc->first_frame + (uint64_t)drawn,
                                               desc->scale, desc->shift, desc->codeword_packed, rm, s))
                return rc;
            if (int rc = ldpc_decode(d, llr, frames, 1, nullptr, nullptr, iters, success, packed, base + w.o_dec, w.dec_bytes, s))
                return rc;
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

}  // namespace

extern "C" {

int ldpc_channel_awgn(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                      float scale, float shift, const uint8_t *codeword_packed, void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (batch == 0) return LDPC_OK;
    if (!llr) return fail(LDPC_ERR_ARG, "NULL llr");
    if (((uintptr_t)llr % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "llr must be 4-byte aligned");
    return sim_channel_launch((float *)llr, batch, n, seed, stream_id, first_frame, scale, shift, codeword_packed,
                              (hipStream_t)stream);
}

int ldpc_channel_awgn_mix(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                          const float *scale_tab, const float *shift_tab, int32_t n_points, const uint8_t *codeword_packed,
                          void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (batch > INT32_MAX) return fail(LDPC_ERR_ARG, "batch > 2^31 - 1");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (n_points < 1 || n_points > 4096) return fail(LDPC_ERR_ARG, "n_points must be in 1 .. 4096");
    if (batch > 0 && first_frame > (uint64_t)0 - (uint64_t)batch)       // 2^64 - batch: p is not continuous across the wrap
        return fail(LDPC_ERR_ARG, "first_frame + batch wraps the 64-bit frame index");
    if (batch == 0) return LDPC_OK;
    if (!llr) return fail(LDPC_ERR_ARG, "NULL llr");
    if (((uintptr_t)llr % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "llr must be 4-byte aligned");
    if (!scale_tab || !shift_tab) return fail(LDPC_ERR_ARG, "NULL scale_tab / shift_tab");
    if (((uintptr_t)scale_tab % sizeof(float)) != 0 || ((uintptr_t)shift_tab % sizeof(float)) != 0)
        return fail(LDPC_ERR_ARG, "scale_tab / shift_tab must be 4-byte aligned");
    return sim_channel_mix_launch((float *)llr, batch, n, seed, stream_id, first_frame, scale_tab, shift_tab, n_points,
                                  codeword_packed, (hipStream_t)stream);
}

int ldpc_sim_count(int64_t *state, const uint8_t *packed_bits, const int32_t *iterations, int64_t batch, int32_t n,
                   const uint8_t *codeword_packed, int64_t max_frames, int64_t max_errors, void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (!state) return fail(LDPC_ERR_ARG, "NULL state");
    if (((uintptr_t)state % sizeof(int64_t)) != 0) return fail(LDPC_ERR_ARG, "state must be 8-byte aligned");
    if (batch > 0 && (!packed_bits || !iterations)) return fail(LDPC_ERR_ARG, "NULL packed_bits / iterations");
    return sim_count_launch(state, packed_bits, iterations, batch, n, codeword_packed, max_frames, max_errors,
                            (hipStream_t)stream);
}

size_t ldpc_simulate_workspace_bytes(const ldpc_decoder *d, int64_t block)
{
    if (!d || block < 1) return 0;
    return sim_carve(d, block).total;
}

int ldpc_simulate(const ldpc_decoder *d, const ldpc_sim_desc *desc, int64_t out_state[8], void *workspace,
                  size_t workspace_bytes, void *stream)
{
    LDPC_NOTHROW(simulate_impl(d, desc, nullptr, -1, out_state, nullptr, workspace, workspace_bytes, stream))
}

size_t ldpc_sim_diag_words(int32_t T, int64_t capture) { return sim_diag_words(T, capture); }

size_t ldpc_sim_count_diag_scratch_bytes(int64_t batch) { return sim_diag_scratch_bytes(batch); }

int ldpc_sim_count_diag(int64_t *state, int64_t *diag, int32_t T, int64_t capture, const uint8_t *packed_bits,
                        const int32_t *iterations, const uint8_t *success, int64_t batch, int32_t n,
                        const uint8_t *codeword_packed, uint64_t block_first_frame, int64_t max_frames, int64_t max_errors,
                        void *scratch, size_t scratch_bytes, void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (T < 0) return fail(LDPC_ERR_ARG, "T < 0");
    if (capture < 0) return fail(LDPC_ERR_ARG, "capture < 0");
    if (sim_diag_words(T, capture) == 0) return fail(LDPC_ERR_ARG, "capture too large");
    if (!state) return fail(LDPC_ERR_ARG, "NULL state");
    if (((uintptr_t)state % sizeof(int64_t)) != 0) return fail(LDPC_ERR_ARG, "state must be 8-byte aligned");
    if (((uintptr_t)diag % sizeof(int64_t)) != 0) return fail(LDPC_ERR_ARG, "diag must be 8-byte aligned");
    if (batch > 0 && (!packed_bits || !iterations || !success)) return fail(LDPC_ERR_ARG, "NULL packed_bits / iterations / success");
    if (batch > 0 && (!diag || !scratch)) return fail(LDPC_ERR_ARG, "NULL diag / scratch");
    if (((uintptr_t)scratch % sizeof(uint32_t)) != 0) return fail(LDPC_ERR_ARG, "scratch must be 4-byte aligned");
    if (scratch_bytes < sim_diag_scratch_bytes(batch))
        return fail(LDPC_ERR_WORKSPACE, "scratch %zu < required %zu", scratch_bytes, sim_diag_scratch_bytes(batch));
    return sim_count_diag_launch(state, diag, T, capture, packed_bits, iterations, success, batch, n, codeword_packed,
                                 block_first_frame, max_frames, max_errors, (uint32_t *)scratch, (hipStream_t)stream);
}

size_t ldpc_simulate_diag_workspace_bytes(const ldpc_decoder *d, int64_t block, int64_t capture)
{
    if (!d || block < 1 || capture < 0 || sim_diag_words(d->T, capture) == 0) return 0;
    return sim_carve(d, block, capture).total;
}

int ldpc_simulate_diag(const ldpc_decoder *d, const ldpc_sim_desc *desc, int64_t capture, int64_t out_state[8],
                       int64_t *out_diag, void *workspace, size_t workspace_bytes, void *stream)
{
    if (capture < 0) return fail(LDPC_ERR_ARG, "capture < 0");
    LDPC_NOTHROW(simulate_impl(d, desc, nullptr, capture, out_state, out_diag, workspace, workspace_bytes, stream))
}

// ---- rate matching: each entry point above with a profile (NULL: the plain call, the very same kernels)
int ldpc_channel_awgn_rm(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                         float scale, float shift, const uint8_t *codeword_packed, const ldpc_rate_match *rm, void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (int rc = sim_rm_check(rm)) return rc;
    if (batch == 0) return LDPC_OK;
    if (!llr) return fail(LDPC_ERR_ARG, "NULL llr");
    if (((uintptr_t)llr % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "llr must be 4-byte aligned");
    return sim_channel_rm_launch((float *)llr, batch, n, seed, stream_id, first_frame, scale, shift, codeword_packed, rm,
                                 (hipStream_t)stream);
}

int ldpc_channel_awgn_mix_rm(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                             const float *scale_tab, const float *shift_tab, int32_t n_points, const uint8_t *codeword_packed,
                             const ldpc_rate_match *rm, void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (batch > INT32_MAX) return fail(LDPC_ERR_ARG, "batch > 2^31 - 1");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (n_points < 1 || n_points > 4096) return fail(LDPC_ERR_ARG, "n_points must be in 1 .. 4096");
    if (batch > 0 && first_frame > (uint64_t)0 - (uint64_t)batch)       // 2^64 - batch: p is not continuous across the wrap
        return fail(LDPC_ERR_ARG, "first_frame + batch wraps the 64-bit frame index");
    if (int rc = sim_rm_check(rm)) return rc;
    if (batch == 0) return LDPC_OK;
    if (!llr) return fail(LDPC_ERR_ARG, "NULL llr");
    if (((uintptr_t)llr % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "llr must be 4-byte aligned");
    if (!scale_tab || !shift_tab) return fail(LDPC_ERR_ARG, "NULL scale_tab / shift_tab");
    if (((uintptr_t)scale_tab % sizeof(float)) != 0 || ((uintptr_t)shift_tab % sizeof(float)) != 0)
        return fail(LDPC_ERR_ARG, "scale_tab / shift_tab must be 4-byte aligned");
    return sim_channel_mix_rm_launch((float *)llr, batch, n, seed, stream_id, first_frame, scale_tab, shift_tab, n_points,
                                     codeword_packed, rm, (hipStream_t)stream);
}

int ldpc_sim_count_rm(int64_t *state, const uint8_t *packed_bits, const int32_t *iterations, int64_t batch, int32_t n,
                      const uint8_t *codeword_packed, int64_t max_frames, int64_t max_errors, const ldpc_rate_match *rm,
                      void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (int rc = sim_rm_check(rm)) return rc;
    if (!state) return fail(LDPC_ERR_ARG, "NULL state");
    if (((uintptr_t)state % sizeof(int64_t)) != 0) return fail(LDPC_ERR_ARG, "state must be 8-byte aligned");
    if (batch > 0 && (!packed_bits || !iterations)) return fail(LDPC_ERR_ARG, "NULL packed_bits / iterations");
    return sim_count_launch(state, packed_bits, iterations, batch, n, codeword_packed, max_frames, max_errors,
                            (hipStream_t)stream, rm ? rm->count_packed : nullptr);
}

int ldpc_sim_count_diag_rm(int64_t *state, int64_t *diag, int32_t T, int64_t capture, const uint8_t *packed_bits,
                           const int32_t *iterations, const uint8_t *success, int64_t batch, int32_t n,
                           const uint8_t *codeword_packed, uint64_t block_first_frame, int64_t max_frames, int64_t max_errors,
                           void *scratch, size_t scratch_bytes, const ldpc_rate_match *rm, void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (T < 0) return fail(LDPC_ERR_ARG, "T < 0");
    if (capture < 0) return fail(LDPC_ERR_ARG, "capture < 0");
    if (sim_diag_words(T, capture) == 0) return fail(LDPC_ERR_ARG, "capture too large");
    if (int rc = sim_rm_check(rm)) return rc;
    if (!state) return fail(LDPC_ERR_ARG, "NULL state");
    if (((uintptr_t)state % sizeof(int64_t)) != 0) return fail(LDPC_ERR_ARG, "state must be 8-byte aligned");
    if (((uintptr_t)diag % sizeof(int64_t)) != 0) return fail(LDPC_ERR_ARG, "diag must be 8-byte aligned");
    if (batch > 0 && (!packed_bits || !iterations || !success)) return fail(LDPC_ERR_ARG, "NULL packed_bits / iterations / success");
    if (batch > 0 && (!diag || !scratch)) return fail(LDPC_ERR_ARG, "NULL diag / scratch");
    if (((uintptr_t)scratch % sizeof(uint32_t)) != 0) return fail(LDPC_ERR_ARG, "scratch must be 4-byte aligned");
    if (scratch_bytes < sim_diag_scratch_bytes(batch))
        return fail(LDPC_ERR_WORKSPACE, "scratch %zu < required %zu", scratch_bytes, sim_diag_scratch_bytes(batch));
    return sim_count_diag_launch(state, diag, T, capture, packed_bits, iterations, success, batch, n, codeword_packed,
                                 block_first_frame, max_frames, max_errors, (uint32_t *)scratch, (hipStream_t)stream,
                                 rm ? rm->count_packed : nullptr);
}

int ldpc_simulate_rm(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_rate_match *rm, int64_t out_state[8],
                     void *workspace, size_t workspace_bytes, void *stream)
{
    LDPC_NOTHROW(simulate_impl(d, desc, rm, -1, out_state, nullptr, workspace, workspace_bytes, stream))
}

int ldpc_simulate_diag_rm(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_rate_match *rm, int64_t capture,
                          int64_t out_state[8], int64_t *out_diag, void *workspace, size_t workspace_bytes, void *stream)
{
    if (capture < 0) return fail(LDPC_ERR_ARG, "capture < 0");
    LDPC_NOTHROW(simulate_impl(d, desc, rm, capture, out_state, out_diag, workspace, workspace_bytes, stream))
}

int ldpc_debug_philox(uint32_t *out4, int64_t count, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                      int32_t quads_per_frame, void *stream)
{
    if (count < 0 || quads_per_frame < 1) return fail(LDPC_ERR_ARG, "bad argument");
    if (count == 0) return LDPC_OK;
    if (!out4) return fail(LDPC_ERR_ARG, "NULL out4");
    const long long blocks = (count + kSimBlock - 1) / kSimBlock;
    if (blocks > 0x7fffffffll) return fail(LDPC_ERR_UNSUPPORTED, "count too large for one launch");
    hipLaunchKernelGGL(sim_debug_philox, dim3((unsigned)blocks), dim3(kSimBlock), 0, (hipStream_t)stream, out4, (long long)count,
                       (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, (unsigned long long)first_frame,
                       (unsigned)quads_per_frame);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

}  // extern "C"
