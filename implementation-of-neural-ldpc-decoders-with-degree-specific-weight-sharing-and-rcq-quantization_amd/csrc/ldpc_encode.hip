// ldpc_encode.hip -- Monte-Carlo on random codewords: the device encoder (ldpc_encoder_create / ldpc_encode /
// ldpc_encode_random), the channel that reads one codeword row per frame (ldpc_channel_awgn_cw) and the host loop of one SNR
// point on them (ldpc_simulate_enc) of include/ldpc_hip.h.
//
// Included by ldpc_hip.hip below ldpc_sim.hip (it uses that file's Philox rounds, channel helpers, counters and workspace
// carving): still the one compiled unit.
//
// Information-bit stream ("Information-bit stream").  Information bit i of frame f is bit i % 32 of word
// x[(i / 32) % 4] of
//   Philox4x32-10(counter = (f & 0xffffffff, f >> 32, 0x80000000 | (i / 128), stream_id), key = (seed & 0xffffffff, seed >> 32)).
// The noise stream's third counter word is a quad index below 2^29 + 256, so the set top bit keeps the two streams disjoint
// under one (seed, stream_id).  A frame's bits are a function of f alone: the codeword of frame f does not depend on the block
// it is drawn in.

namespace ldpc {

constexpr int kEncWaves = kSimBlock / 64;       // one wave per frame, four frames per workgroup

// geometry of one wave's LDS slice, in 32-bit words: information words, parity words (64 rows per pair), the assembled row
struct EncGeom {
    int n, k, m;
    int wk, wp, wn;                             // ceil(k / 32), 2 * ceil(m / 64), ceil(n / 32) + 1 (one zero word behind the row)
    int accumulate, systematic;
    __host__ __device__ int words() const { return wk + wp + wn; }
};

// 32 bits of a packed bit string of `words` words starting at bit s (s >= -31); bits outside the string read 0
__device__ inline uint32_t enc_bits_at(const uint32_t *w, int words, int s)
{
    if (s < 0) return w[0] << (-s);
    const int idx = s >> 5, sh = s & 31;
    const uint32_t lo = idx < words ? w[idx] : 0u, hi = idx + 1 < words ? w[idx + 1] : 0u;
    return sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
}

// `bytes` bytes of the LDS word string src to dst, by one wave: byte stores up to the first 4-byte aligned address, 32-bit
// stores of the realigned words, byte stores for the tail.  src has one readable word behind its last used one.
__device__ inline void enc_store_row(uint8_t *__restrict__ dst, const uint32_t *src, int bytes, int lane)
{
    int head = (int)((4u - (unsigned)((uintptr_t)dst & 3u)) & 3u);
    if (head > bytes) head = bytes;
    const int mid = (bytes - head) >> 2, tail0 = head + 4 * mid;
    if (lane < head) dst[lane] = (uint8_t)(src[0] >> (8 * lane));
    for (int d = lane; d < mid; d += 64) {
        const int o = head + 4 * d, idx = o >> 2, sh = 8 * (o & 3);
        const uint32_t v = sh ? (src[idx] >> sh) | (src[idx + 1] << (32 - sh)) : src[idx];
        *reinterpret_cast<uint32_t *>(dst + o) = v;
    }
    if (lane < bytes - tail0) {
        const int o = tail0 + lane;
        dst[o] = (uint8_t)(src[o >> 2] >> (8 * (o & 3)));
    }
}

// One wave encodes one frame; the workgroup's four waves share nothing but the barriers (every wave runs every barrier: the
// trip counts depend on the geometry only, a wave past the batch just stores nothing).
//   1. information words into LDS: drawn (lane c runs the Philox call of words 4c .. 4c + 3) or read from info_in
//   2. parity rows, 64 at a time: each lane XORs its row's information bits out of LDS, a ballot packs the 64 results; with
//      `accumulate` the prefix XOR inside the word is the six-step shift-XOR ladder on the wave-uniform ballot word and the
//      carry into the next word is its top bit -- the words of a frame are walked in order by the one wave anyway
//   3. the row: information words then the parity string shifted by k % 32 (systematic), or every set bit scattered to its
//      position with an LDS atomic OR
//   4. stores of the width the address allows (rows are ceil(n / 8) bytes apart: no alignment to rely on)
__global__ __launch_bounds__(kSimBlock) void enc_encode(EncGeom g, const int *__restrict__ info_pos,
                                                        const int *__restrict__ parity_pos, const int *__restrict__ row_ptr,
                                                        const int *__restrict__ info_idx, long long batch, int random,
                                                        uint32_t k0, uint32_t k1, uint32_t stream_id,
                                                        unsigned long long first_frame, const uint8_t *__restrict__ info_in,
                                                        uint8_t *__restrict__ cw_out, uint8_t *__restrict__ info_out)
{
    extern __shared__ uint32_t enc_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t *info = enc_lds + (size_t)wv * g.words();
    uint32_t *par = info + g.wk;
    uint32_t *row = par + g.wp;
    const long long b = (long long)blockIdx.x * kEncWaves + wv;
    const bool live = b < batch;
    const int kb = (g.k + 7) >> 3, nb = (g.n + 7) >> 3;

    // 1. information words; bits at and beyond k are zero
    if (random) {
        const unsigned long long f = first_frame + (unsigned long long)b;
        for (int c = lane; 4 * c < g.wk; c += 64) {
            uint32_t x[4];
            philox4x32_10((uint32_t)f, (uint32_t)(f >> 32), 0x80000000u | (uint32_t)c, stream_id, k0, k1, x);
            for (int j = 0; j < 4; ++j)
                if (4 * c + j < g.wk) info[4 * c + j] = x[j];
        }
    } else {
        const uint8_t *src = info_in + (size_t)(live ? b : 0) * (size_t)kb;
        for (int w = lane; w < g.wk; w += 64) info[w] = live ? sim_row_word(src, kb, 4 * w) : 0u;
    }
    __syncthreads();
    if ((g.k & 31) && lane == 0) info[g.wk - 1] &= (1u << (g.k & 31)) - 1u;
    __syncthreads();
    if (info_out && live) {
        // the information row is followed by one readable word: par[0] when m > 0, else row[0]
        enc_store_row(info_out + (size_t)b * (size_t)kb, info, kb, lane);
    }

    // 2. parity words
    unsigned long long carry = 0;
    for (int base = 0; base < g.m; base += 64) {
        const int r = base + lane;
        unsigned bit = 0;
        if (r < g.m) {
            const int e1 = row_ptr[r + 1];
            for (int e = row_ptr[r]; e < e1; ++e) {
                const int i = info_idx[e];
                bit ^= info[i >> 5] >> (i & 31);
            }
        }
        unsigned long long w = __ballot(bit & 1u);
        if (g.accumulate) {
            w ^= w << 1; w ^= w << 2; w ^= w << 4; w ^= w << 8; w ^= w << 16; w ^= w << 32;
            if (carry) w = ~w;
            carry = w >> 63;
        }
        if (g.m - base < 64) w &= (1ull << (g.m - base)) - 1ull;
        if (lane == 0) {
            par[base >> 5] = (uint32_t)w;
            par[(base >> 5) + 1] = (uint32_t)(w >> 32);
        }
    }
    __syncthreads();

    // 3. the row in LDS, one zero word behind it
    if (g.systematic) {
        for (int j = lane; j < g.wn; j += 64) {
            uint32_t v = 32 * j < g.k ? info[j] : 0u;
            const int s = 32 * j - g.k;                      // first parity bit of this word
            if (s > -32 && s < g.m) v |= enc_bits_at(par, g.wp, s);
            row[j] = v;
        }
        __syncthreads();
    } else {
        for (int j = lane; j < g.wn; j += 64) row[j] = 0u;
        __syncthreads();
        for (int i = lane; i < g.k; i += 64)
            if ((info[i >> 5] >> (i & 31)) & 1u) {
                const int p = info_pos[i];
                atomicOr(&row[p >> 5], 1u << (p & 31));
            }
        for (int r = lane; r < g.m; r += 64)
            if ((par[r >> 5] >> (r & 31)) & 1u) {
                const int p = parity_pos[r];
                atomicOr(&row[p >> 5], 1u << (p & 31));
            }
        __syncthreads();
    }

    // 4. out
    if (live) enc_store_row(cw_out + (size_t)b * (size_t)nb, row, nb, lane);
}

// ldpc_channel_awgn_cw: sim_channel_awgn (RM = false) / sim_channel_awgn_rm (RM = true) with the codeword bits of frame b read
// from row b of cw[batch][ceil(n / 8)].  The same lane-per-quad shape, counters, normals, operations in the same order and
// stores: frame b equals the one-codeword kernel's draw of that frame with that row, bit for bit.
template <bool RM>
__global__ __launch_bounds__(kSimBlock) void sim_channel_awgn_cw(float *__restrict__ llr, long long batch, int n, unsigned Q,
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
    const uint8_t *cwrow = cw + (size_t)b * (size_t)((n + 7) >> 3);
    const unsigned long long f = first_frame + (unsigned long long)b;
    float v[4];
    if (RM) {
        unsigned cbits, pbits, sbits;
        sim_rm_nibbles(j0, cwrow, punct, shrt, cbits, pbits, sbits);
        sim_rm_quad(f, q, k0, k1, stream_id, scale, shift, short_llr, cbits, pbits, sbits, (1u << cnt) - 1u, v);
    } else {
        const unsigned cbits = (cwrow[j0 >> 3] >> (j0 & 7)) & 0xfu;               // j0 % 8 is 0 or 4: one byte holds all four
        uint32_t x[4];
        philox4x32_10((uint32_t)f, (uint32_t)(f >> 32), q, stream_id, k0, k1, x);
        float z[4];
        sim_box_muller(x[0], x[1], z[0], z[1]);
        sim_box_muller(x[2], x[3], z[2], z[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float y = fmaf(z[k], scale, shift);
            v[k] = ((cbits >> k) & 1u) ? -y : y;
        }
    }
    sim_store_quad(llr + (size_t)b * (size_t)n + (size_t)j0, v, cnt);
}

// packed[i] ^= cw[i] over `bytes` bytes: the decisions of a block unscrambled by the codewords that were sent.  Both buffers
// start 4-byte aligned (workspace slices): 32-bit words, then the last bytes one by one.
__global__ __launch_bounds__(kSimBlock) void enc_xor_rows(uint8_t *__restrict__ packed, const uint8_t *__restrict__ cw,
                                                          long long bytes)
{
    const long long words = bytes >> 2;
    const long long i = (long long)blockIdx.x * kSimBlock + threadIdx.x;
    if (i < words) reinterpret_cast<uint32_t *>(packed)[i] ^= reinterpret_cast<const uint32_t *>(cw)[i];
    const long long t = 4 * words + i;
    if (i < 4 && t < bytes) packed[t] ^= cw[t];
}

}  // namespace ldpc

struct ldpc_encoder {
    int device = 0;
    EncGeom g{};
    int *info_pos = nullptr, *parity_pos = nullptr, *row_ptr = nullptr, *info_idx = nullptr;
    size_t lds = 0;                             // dynamic LDS of one enc_encode workgroup
};

namespace {

constexpr size_t kEncMaxLds = 64 * 1024;

int encoder_create_impl(ldpc_encoder **out, int32_t n, int32_t k, const int32_t *info_pos, const int32_t *parity_pos,
                        const int32_t *row_ptr, const int32_t *info_idx, int32_t accumulate)
{
    if (!out) return fail(LDPC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (n < 1 || k < 0 || k > n) return fail(LDPC_ERR_ARG, "need n >= 1 and 0 <= k <= n");
    const int32_t m = n - k;
    if ((k > 0 && !info_pos) || (m > 0 && !parity_pos) || !row_ptr) return fail(LDPC_ERR_ARG, "NULL info_pos / parity_pos / row_ptr");
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int part = 0; part < 2; ++part) {
        const int32_t *pos = part ? parity_pos : info_pos;
        const int32_t cnt = part ? m : k;
        for (int32_t i = 0; i < cnt; ++i) {
            const int32_t p = pos[i];
            if (p < 0 || p >= n) return fail(LDPC_ERR_ARG, "%s[%d]=%d out of range", part ? "parity_pos" : "info_pos", i, p);
            if (seen[p]) return fail(LDPC_ERR_ARG, "info_pos and parity_pos are not a permutation: position %d twice", p);
            seen[p] = 1;
        }
    }
    if (row_ptr[0] != 0) return fail(LDPC_ERR_ARG, "row_ptr[0] must be 0");
    for (int32_t r = 0; r < m; ++r)
        if (row_ptr[r + 1] < row_ptr[r]) return fail(LDPC_ERR_ARG, "row_ptr not monotone at row %d", r);
    const int32_t E = row_ptr[m];
    if (E > 0 && !info_idx) return fail(LDPC_ERR_ARG, "NULL info_idx");
    for (int32_t e = 0; e < E; ++e)
        if (info_idx[e] < 0 || info_idx[e] >= k) return fail(LDPC_ERR_ARG, "info_idx[%d]=%d out of range", e, info_idx[e]);
    EncGeom g{};
    g.n = n; g.k = k; g.m = m;
    g.wk = (k + 31) / 32;
    g.wp = 2 * ((m + 63) / 64);
    g.wn = (n + 31) / 32 + 1;
    g.accumulate = accumulate != 0;
    g.systematic = 1;
    for (int32_t i = 0; i < k && g.systematic; ++i) g.systematic = info_pos[i] == i;
    for (int32_t r = 0; r < m && g.systematic; ++r) g.systematic = parity_pos[r] == k + r;
    const size_t lds = (size_t)kEncWaves * (size_t)g.words() * sizeof(uint32_t);
    if (lds > kEncMaxLds) return fail(LDPC_ERR_UNSUPPORTED, "a frame of n = %d does not fit the encoder's LDS (%zu > %zu bytes)", n, lds, kEncMaxLds);
    ldpc_encoder *e = new (std::nothrow) ldpc_encoder();
    if (!e) return fail(LDPC_ERR_ARG, "out of host memory");
    e->g = g;
    e->lds = lds;
    if (hipGetDevice(&e->device) != hipSuccess) {
        delete e;
        return fail(LDPC_ERR_HIP, "no HIP device available");
    }
    int rc = upload(&e->info_pos, info_pos, (size_t)k);
    if (!rc) rc = upload(&e->parity_pos, parity_pos, (size_t)m);
    if (!rc) rc = upload(&e->row_ptr, row_ptr, (size_t)m + 1);
    if (!rc) rc = upload(&e->info_idx, E > 0 ? info_idx : nullptr, (size_t)E);
    if (rc) {
        ldpc_encoder_destroy(e);
        return rc;
    }
    *out = e;
    return LDPC_OK;
}

// one launch of enc_encode; the caller has set the device
int enc_launch(const ldpc_encoder *e, int64_t batch, int random, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
               const uint8_t *info_in, uint8_t *cw_out, uint8_t *info_out, hipStream_t s)
{
    const long long blocks = (batch + kEncWaves - 1) / kEncWaves;
    if (blocks > 0x7fffffffll) return fail(LDPC_ERR_UNSUPPORTED, "batch too large for one launch");
    hipLaunchKernelGGL(enc_encode, dim3((unsigned)blocks), dim3(kSimBlock), e->lds, s, e->g, (const int *)e->info_pos,
                       (const int *)e->parity_pos, (const int *)e->row_ptr, (const int *)e->info_idx, (long long)batch, random,
                       (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, (unsigned long long)first_frame, info_in, cw_out,
                       info_out);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int sim_channel_cw_launch(float *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                          float scale, float shift, const uint8_t *cw, const ldpc_rate_match *rm, hipStream_t s)
{
    const unsigned Q = ((unsigned)n + 3u) / 4u;
    const unsigned long long quads = (unsigned long long)batch * Q;
    const unsigned long long blocks = (quads + kSimBlock - 1) / kSimBlock;
    if (blocks > 0x7fffffffull) return fail(LDPC_ERR_UNSUPPORTED, "batch too large for one launch");
    if (rm)
        hipLaunchKernelGGL(sim_channel_awgn_cw<true>, dim3((unsigned)blocks), dim3(kSimBlock), 0, s, llr, (long long)batch,
                           (int)n, Q, (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, (unsigned long long)first_frame, scale,
                           shift, cw, rm->punctured_packed, rm->shortened_packed,
                           rm->shortened_packed ? rm->short_llr : 0.0f);
    else
        hipLaunchKernelGGL(sim_channel_awgn_cw<false>, dim3((unsigned)blocks), dim3(kSimBlock), 0, s, llr, (long long)batch,
                           (int)n, Q, (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, (unsigned long long)first_frame, scale,
                           shift, cw, (const uint8_t *)nullptr, (const uint8_t *)nullptr, 0.0f);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

// workspace of ldpc_simulate_enc: that of ldpc_simulate / _diag with the block's codeword rows behind it
size_t sim_enc_cw_offset(const ldpc_decoder *d, int64_t block, int64_t capture) { return align_up(sim_carve(d, block, capture).total); }

size_t sim_enc_total(const ldpc_decoder *d, int64_t block, int64_t capture)
{
    return sim_enc_cw_offset(d, block, capture) + align_up((size_t)block * (((size_t)d->g->n + 7) / 8));
}

// simulate_impl's loop with a fresh codeword per frame: encode_random, the per-frame channel, ldpc_decode, the decisions
// XORed with the codeword rows, then the existing counters against the all-zero word.  The code is linear: popcount((d ^ c) &
// mask) is the error count, d satisfies H exactly when d ^ c does and `success` comes from the decoder, so neither the counter
// nor the diagnostic kernels need a per-frame form.
int simulate_enc_impl(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_encoder *e, const ldpc_rate_match *rm,
                      int64_t capture, int64_t out_state[8], int64_t *out_diag, void *workspace, size_t workspace_bytes,
                      void *stream)
{
    const bool diagnostics = capture >= 0;
    if (!d || !desc || !e || !out_state) return fail(LDPC_ERR_ARG, "NULL decoder / descriptor / encoder / out_state");
    if (diagnostics && !out_diag) return fail(LDPC_ERR_ARG, "NULL out_diag");
    if (diagnostics && sim_diag_words(d->T, capture) == 0) return fail(LDPC_ERR_ARG, "capture too large");
    if (int rc = sim_rm_check(rm)) return rc;
    const uint8_t *mask = rm ? rm->count_packed : nullptr;
    if (desc->codeword_packed) return fail(LDPC_ERR_ARG, "codeword_packed must be NULL: the codewords are drawn per frame");
    if (desc->block < 1) return fail(LDPC_ERR_ARG, "block < 1");
    if (desc->poll_blocks < 1) return fail(LDPC_ERR_ARG, "poll_blocks < 1");
    if (d->dtype != LDPC_F32) return fail(LDPC_ERR_UNSUPPORTED, "ldpc_simulate_enc draws fp32 LLRs: float64 decoders are not supported");
    if (d->g->n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (e->g.n != d->g->n) return fail(LDPC_ERR_ARG, "the encoder has n = %d, the decoder n = %d", e->g.n, d->g->n);
    if (e->device != d->g->device) return fail(LDPC_ERR_ARG, "encoder and decoder live on different devices");
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
    PinnedState host;
    HIP_TRY(hipHostMalloc((void **)&host.p, 8 * sizeof(int64_t), hipHostMallocDefault));
    HIP_TRY(hipMemsetAsync(state, 0, 8 * sizeof(int64_t), s));
    if (diagnostics) HIP_TRY(hipMemsetAsync(diag, 0, w.diag_words * sizeof(int64_t), s));
    auto count = [&](int64_t frames, int64_t first) {    // fold one unscrambled block (frames = 0: latch `done`)
        if (diagnostics)
            return sim_count_diag_launch(state, diag, d->T, capture, packed, iters, success, frames, n, nullptr,
                                         desc->first_frame + (uint64_t)first, desc->max_frames, desc->max_errors, words, s, mask);
        return sim_count_launch(state, packed, iters, frames, n, nullptr, desc->max_frames, desc->max_errors, s, mask);
    };
    int64_t drawn = 0;                                   // frames drawn so far: block k starts at first_frame + k * block
    for (;;) {
        int queued = 0;
        for (int p = 0; p < desc->poll_blocks && drawn < desc->max_frames; ++p, ++queued) {
            const int64_t frames = std::min<int64_t>(desc->block, desc->max_frames - drawn);
            const uint64_t first = desc->first_frame + (uint64_t)drawn;
            if (int rc = enc_launch(e, frames, 1, desc->seed, desc->stream_id, first, nullptr, cw, nullptr, s)) return rc;
            if (int rc = sim_channel_cw_launch(llr, frames, n, desc->seed, desc->stream_id, first, desc->scale, desc->shift, cw,
                                               rm, s))
                return rc;
            if (int rc = ldpc_decode(d, llr, frames, 1, nullptr, nullptr, iters, success, packed, base + w.o_dec, w.dec_bytes, s))
                return rc;
            const long long bytes = (long long)frames * rb, xblocks = ((bytes >> 2) + kSimBlock - 1) / kSimBlock;
            hipLaunchKernelGGL(enc_xor_rows, dim3((unsigned)std::max<long long>(xblocks, 1)), dim3(kSimBlock), 0, s, packed,
                               (const uint8_t *)cw, bytes);
            HIP_TRY(hipGetLastError());
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

int ldpc_encoder_create(ldpc_encoder **out, int32_t n, int32_t k, const int32_t *info_pos, const int32_t *parity_pos,
                        const int32_t *row_ptr, const int32_t *info_idx, int32_t accumulate)
{
    LDPC_NOTHROW(encoder_create_impl(out, n, k, info_pos, parity_pos, row_ptr, info_idx, accumulate))
}

void ldpc_encoder_destroy(ldpc_encoder *e)
{
    if (!e) return;
    DeviceGuard guard(e->device);
    (void)hipFree(e->info_pos); (void)hipFree(e->parity_pos); (void)hipFree(e->row_ptr); (void)hipFree(e->info_idx);
    delete e;
}

int ldpc_encode(const ldpc_encoder *e, const uint8_t *info_packed, int64_t batch, uint8_t *codewords_packed, void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (batch == 0) return LDPC_OK;
    if (!e) return fail(LDPC_ERR_ARG, "NULL encoder");
    if (!codewords_packed || (e->g.k > 0 && !info_packed)) return fail(LDPC_ERR_ARG, "NULL info_packed / codewords_packed");
    DeviceGuard guard(e->device);
    return enc_launch(e, batch, 0, 0, 0, 0, info_packed, codewords_packed, nullptr, (hipStream_t)stream);
}

int ldpc_encode_random(const ldpc_encoder *e, int64_t batch, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                       uint8_t *codewords_packed, uint8_t *info_packed, void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (batch == 0) return LDPC_OK;
    if (!e) return fail(LDPC_ERR_ARG, "NULL encoder");
    if (!codewords_packed) return fail(LDPC_ERR_ARG, "NULL codewords_packed");
    DeviceGuard guard(e->device);
    return enc_launch(e, batch, 1, seed, stream_id, first_frame, nullptr, codewords_packed, info_packed, (hipStream_t)stream);
}

int ldpc_channel_awgn_cw(void *llr, int64_t batch, int32_t n, uint64_t seed, uint32_t stream_id, uint64_t first_frame,
                         float scale, float shift, const uint8_t *codewords_packed, const ldpc_rate_match *rm, void *stream)
{
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (n < 1) return fail(LDPC_ERR_ARG, "n < 1");
    if (int rc = sim_rm_check(rm)) return rc;
    if (batch == 0) return LDPC_OK;
    if (!llr) return fail(LDPC_ERR_ARG, "NULL llr");
    if (((uintptr_t)llr % sizeof(float)) != 0) return fail(LDPC_ERR_ARG, "llr must be 4-byte aligned");
    if (!codewords_packed) return fail(LDPC_ERR_ARG, "NULL codewords_packed");
    return sim_channel_cw_launch((float *)llr, batch, n, seed, stream_id, first_frame, scale, shift, codewords_packed, rm,
                                 (hipStream_t)stream);
}

size_t ldpc_simulate_enc_workspace_bytes(const ldpc_decoder *d, int64_t block, int64_t capture)
{
    if (!d || block < 1) return 0;
    if (capture >= 0 && sim_diag_words(d->T, capture) == 0) return 0;
    return sim_enc_total(d, block, capture < 0 ? -1 : capture);
}

int ldpc_simulate_enc(const ldpc_decoder *d, const ldpc_sim_desc *desc, const ldpc_encoder *e, const ldpc_rate_match *rm,
                      int64_t capture, int64_t out_state[8], int64_t *out_diag, void *workspace, size_t workspace_bytes,
                      void *stream)
{
    LDPC_NOTHROW(simulate_enc_impl(d, desc, e, rm, capture < 0 ? -1 : capture, out_state, out_diag, workspace, workspace_bytes,
                                   stream))
}

}  // extern "C"
